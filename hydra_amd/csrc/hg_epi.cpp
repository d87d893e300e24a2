// hg_epi.cpp -- BOOST's interaction test of one pair of markers from its 2 x 3 x 3 table, for --epistasis: plain
// C++, no HIP, no handle.
//
//     int hgibbs_epi_test(const int32_t* table18, hgibbs_epi_result* r);
//
//   table    table18[9 k + 3 i + j] = n_ijk >= 0: class k, code i of the first marker, code j of the second (hgibbs_pair_tables' layout)
//   ksa      the Kirkwood superposition bound (hg_epi_math.h: the same operations as the device's screen)
//   df       (I - 1)(J - 1), I and J the codes of each marker that occur in the table: 0, 1, 2 or 4
//   lr       2 (L_S - L_H) = 2 sum_{n_ijk > 0} n_ijk (log(n_ijk / n) - log(m_ijk / n)), k, i, j ascending, not below 0; m the fit of the
//            homogeneous-association model (all three two-way margins, no three-way term) by iterative proportional fitting:
//              start    m_ijk = 1
//              cycle    ij: m_ijk *= n_ij. / (m_ij0 + m_ij1);   ik: m_ijk *= n_i.k / ((m_i0k + m_i1k) + m_i2k);
//                       jk: m_ijk *= n_.jk / ((m_0jk + m_1jk) + m_2jk);   a margin of m that is 0 leaves its cells at 0
//              stop     after the cycle in which no cell moved by more than EPI_TOL n = 1e-10 n (converged = 1), or after EPI_CYCLES =
//                       2000 cycles (converged = 0: the likelihood of m is below the maximum, so lr is an upper bound of the statistic)
//            df = 0: the model is saturated, lr = 0 exactly, iters = 0, converged = 1, p = NaN
//   p        the chi-square upper tail in closed form: erfc(sqrt(x / 2)), exp(-x / 2), exp(-x / 2) (1 + x / 2) for df = 1, 2, 4
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../include/hgibbs.h"
#include "hg_epi_math.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

constexpr double EPI_TOL = 1e-10;
constexpr int EPI_CYCLES = 2000;

} // namespace

extern "C" int hgibbs_epi_test(const int32_t* t, hgibbs_epi_result* r)
{
    if (!t || !r) {
        hgibbs_set_error_("hgibbs_epi_test: null argument");
        return 1;
    }
    for (int c = 0; c < 18; ++c)
        if (t[c] < 0) {
            char msg[128];
            std::snprintf(msg, sizeof msg, "hgibbs_epi_test: table[%d] = %d is negative", c, (int)t[c]);
            hgibbs_set_error_(msg);
            return 1;
        }
    r->ksa = hg_epi_ksa(t, nullptr);
    long long nij[9], nik[6], njk[6], n = 0;
    int I = 0, J = 0;
    for (int c = 0; c < 9; ++c) nij[c] = (long long)t[c] + t[9 + c];
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 3; ++i) {
            nik[3 * k + i] = (long long)t[9 * k + 3 * i] + t[9 * k + 3 * i + 1] + t[9 * k + 3 * i + 2];
            njk[3 * k + i] = (long long)t[9 * k + i] + t[9 * k + 3 + i] + t[9 * k + 6 + i];
            n += nik[3 * k + i];
        }
    for (int i = 0; i < 3; ++i) {
        I += nik[i] + nik[3 + i] > 0;
        J += njk[i] + njk[3 + i] > 0;
    }
    r->df = I && J ? (I - 1) * (J - 1) : 0;
    r->lr = 0.0;
    r->iters = 0;
    r->converged = 1;
    r->p = std::numeric_limits<double>::quiet_NaN();
    if (r->df == 0) return 0;

    double m[18], old[18];
    for (int c = 0; c < 18; ++c) m[c] = 1.0;
    const double lim = EPI_TOL * (double)n;
    r->converged = 0;
    while (r->iters < EPI_CYCLES) {
        for (int c = 0; c < 18; ++c) old[c] = m[c];
        for (int c = 0; c < 9; ++c) {
            const double s = m[c] + m[9 + c], f = s > 0.0 ? (double)nij[c] / s : 0.0;
            m[c] *= f;
            m[9 + c] *= f;
        }
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 3; ++i) {
                double* row = m + 9 * k + 3 * i;
                const double s = (row[0] + row[1]) + row[2], f = s > 0.0 ? (double)nik[3 * k + i] / s : 0.0;
                row[0] *= f;
                row[1] *= f;
                row[2] *= f;
            }
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 3; ++j) {
                double* col = m + 9 * k + j;
                const double s = (col[0] + col[3]) + col[6], f = s > 0.0 ? (double)njk[3 * k + j] / s : 0.0;
                col[0] *= f;
                col[3] *= f;
                col[6] *= f;
            }
        ++r->iters;
        double d = 0.0;
        for (int c = 0; c < 18; ++c) d = std::fmax(d, std::fabs(m[c] - old[c]));
        if (d <= lim) {
            r->converged = 1;
            break;
        }
    }
    double s = 0.0;
    for (int c = 0; c < 18; ++c) {
        if (t[c] <= 0) continue;
        const double x = (double)t[c];
        s += x * (std::log(x / (double)n) - std::log(m[c] / (double)n));
    }
    const double x = std::fmax(2.0 * s, 0.0);
    r->lr = x;
    r->p = r->df == 1 ? std::erfc(std::sqrt(x / 2.0)) : r->df == 2 ? std::exp(-x / 2.0) : std::exp(-x / 2.0) * (1.0 + x / 2.0);
    return 0;
}
