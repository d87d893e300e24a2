// shuffle_bench.cpp -- host-only timing of the marker shuffle (hg_rng.h): the sequential definition against the fast
// form, each checked for the identical permutation and generator state.
//   clang++ -O3 -std=c++17 -ffp-contract=off -o shuffle_bench tools/shuffle_bench.cpp && ./shuffle_bench [n] [reps]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../hydra_amd/csrc/hg_rng.h"

namespace {
struct State {
    uint32_t x[hg::MT_N];
    uint32_t idx;
};

template <class F>
void run(const char* name, size_t n, int reps, const std::vector<int32_t>& want, const State& want_st, F f)
{
    double best = 1e30, sum = 0.0;
    bool same = true;
    for (int r = 0; r < reps; ++r) {
        State s;
        hg::Mt g{s.x, 0};
        g.seed(1222);
        std::vector<int32_t> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = (int32_t)i;
        const auto t0 = std::chrono::steady_clock::now();
        f(v.data(), n, g); // two in a row, as the chain does across iterations (the second on a shuffled array)
        f(v.data(), n, g);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / 2;
        best = ms < best ? ms : best;
        sum += ms;
        s.idx = g.idx;
        same = same && v == want && !std::memcmp(s.x, want_st.x, sizeof s.x) && s.idx == want_st.idx;
    }
    std::printf("%-34s best %8.3f ms  mean %8.3f ms per shuffle  %s\n", name, best, sum / reps, same ? "identical" : "DIFFERENT");
}
} // namespace

int main(int argc, char** argv)
{
    const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1000000;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 7;
    State ws;
    std::vector<int32_t> want(n);
    {
        hg::Mt g{ws.x, 0};
        g.seed(1222);
        for (size_t i = 0; i < n; ++i) want[i] = (int32_t)i;
        hg::shuffle_libstdcxx6(want.data(), n, g);
        hg::shuffle_libstdcxx6(want.data(), n, g);
        ws.idx = g.idx;
    }
    std::printf("n = %zu, %d repetitions\n", n, reps);
    run("sequential (definition)", n, reps, want, ws, [](int32_t* v, size_t m, hg::Mt& g) { hg::shuffle_libstdcxx6(v, m, g); });
    run("fast", n, reps, want, ws, [](int32_t* v, size_t m, hg::Mt& g) { hg::shuffle_libstdcxx6_fast(v, m, g); });
    return 0;
}
