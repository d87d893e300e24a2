// hg_ldgreedy.cpp -- the greedy selection on the LD masks of hgibbs_ld_mask: plain C++, no HIP.
//
// Walk the participating markers in their order of priority; a marker nobody owns yet, and that may lead, becomes a leader and claims
// every participating, unowned marker whose pair with it passes (PLINK's clump walk).  The chain of dependencies is as long as M when
// the priority follows the .bim order and every step is a handful of word operations, so this stays on the host.
//
// On words: `open` is the bitset of "participating and unowned", marker m at bit m + OFF (OFF = 64 (wpr + 1) bits of zero padding in
// front, as many behind, so that no window read leaves the array or meets a marker that does not exist).  Word k of v's forward row
// covers markers v + 1 + 64 k .. + 63 in ascending order: AND it with the 64 bits of `open` from there.  Word k of v's backward row
// covers markers v - 1 - 64 k downwards: reverse its bits and AND it with the 64 bits of `open` that end there.  Only the set bits of the
// AND are visited: O(M wpr) words in all, not O(M W) probes.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

int gfail(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    hgibbs_set_error_(buf);
    return 1;
}

inline uint64_t rev64(uint64_t x)
{
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}

// the 64 bits of b from bit position pos
inline uint64_t get64(const std::vector<uint64_t>& b, uint64_t pos)
{
    const uint64_t w = pos >> 6, s = pos & 63u;
    return s ? (b[w] >> s) | (b[w + 1] << (64u - s)) : b[w];
}

} // namespace

extern "C" int hgibbs_ld_greedy(uint32_t M, uint32_t W, const uint64_t* fwd, const uint64_t* bwd, const uint32_t* order, uint32_t norder,
                                const uint8_t* may_lead, int32_t* owner)
{
    if (W == 0 || W > 4096u) return gfail("hgibbs_ld_greedy: W = %u, must be in [1, 4096]", W);
    if (M == 0 || M > 0x7FFFFFFFu) return gfail("hgibbs_ld_greedy: M = %u, must be in [1, 2^31 - 1] (owner holds marker indices as int32)", M);
    if (!fwd || !bwd) return gfail("hgibbs_ld_greedy: null mask (%s)", !fwd ? "fwd" : "bwd");
    if (!owner) return gfail("hgibbs_ld_greedy: null output (owner)");
    if (norder && !order) return gfail("hgibbs_ld_greedy: null order with norder = %u", norder);
    const uint32_t wpr = (W + 63u) / 64u;
    const uint64_t OFF = 64ull * (wpr + 1u);
    std::vector<uint64_t> open((2 * OFF + M + 63u) / 64u + 1u, 0ull);
    for (uint32_t k = 0; k < norder; ++k) {
        const uint32_t v = order[k];
        if (v >= M) return gfail("hgibbs_ld_greedy: order[%u] = %u is not below M = %u", k, v, M);
        const uint64_t pos = v + OFF;
        if ((open[pos >> 6] >> (pos & 63u)) & 1ull) return gfail("hgibbs_ld_greedy: order[%u] = %u is in the order twice", k, v);
        open[pos >> 6] |= 1ull << (pos & 63u);
    }
    for (uint32_t j = 0; j < M; ++j) owner[j] = -1;
    const uint64_t last = (W & 63u) ? (1ull << (W & 63u)) - 1ull : ~0ull; // the offsets up to W in a row's last word
    auto claim = [&](uint64_t hits, int64_t first, uint32_t v) { // bit i of hits is marker first + i
        for (; hits; hits &= hits - 1ull) {
            const uint64_t q = (uint64_t)(first + __builtin_ctzll(hits)), pos = q + OFF;
            owner[q] = (int32_t)v;
            open[pos >> 6] &= ~(1ull << (pos & 63u));
        }
    };
    for (uint32_t k = 0; k < norder; ++k) {
        const uint32_t v = order[k];
        if (owner[v] != -1) continue;
        if (may_lead && !may_lead[v]) continue;
        owner[v] = (int32_t)v;
        open[(v + OFF) >> 6] &= ~(1ull << ((v + OFF) & 63u));
        const uint64_t* fr = fwd + (uint64_t)v * wpr;
        const uint64_t* br = bwd + (uint64_t)v * wpr;
        for (uint32_t w = 0; w < wpr; ++w) {
            const uint64_t keep = w + 1u == wpr ? last : ~0ull;
            const uint64_t f = fr[w] & keep, b = br[w] & keep;
            if (f) {
                const int64_t first = (int64_t)v + 1 + 64 * (int64_t)w;
                claim(f & get64(open, (uint64_t)(first + (int64_t)OFF)), first, v);
            }
            if (b) {
                const int64_t first = (int64_t)v - 64 - 64 * (int64_t)w; // bit i of the reversed word is marker first + i
                claim(rev64(b) & get64(open, (uint64_t)(first + (int64_t)OFF)), first, v);
            }
        }
    }
    return 0;
}
