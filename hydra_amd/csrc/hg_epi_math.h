// BOOST's Kirkwood superposition bound of one 2 x 3 x 3 table, in ONE order of operations for the host
// (hg_epi.cpp) and the device (k_epi_screen, hg_pairtab.hip.h).  t[9 k + 3 i + j] = n_ijk: class k, code i of the first marker, code j
// of the second.
//
//     q_ijk = n_ij. n_i.k n_.jk / (n_i.. n_.j. n_..k)      (the n^3 of the six pi cancel; 0 where a margin of the divisor is 0)
//     eta   = sum q_ijk                                     (k, i, j ascending)
//     KSA   = 2 sum_{n_ijk > 0} n_ijk (log(n_ijk / n) - log(q_ijk / eta))      (k, i, j ascending)
//
// The margins are exact integers; every double operation stands here once, so the two sides differ by their log alone.  abs_terms, when
// asked for, is sum n_ijk (|log(n_ijk / n)| + |log(q_ijk / eta)|): the scale the rounding error is relative to.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define HG_EPI_HD __host__ __device__
#else
#define HG_EPI_HD
#endif

HG_EPI_HD inline double hg_epi_ksa(const int32_t* t, double* abs_terms)
{
    long long nij[9], nik[6], njk[6], ni[3] = {0, 0, 0}, nj[3] = {0, 0, 0}, nk[2] = {0, 0}, n = 0;
    for (int c = 0; c < 9; ++c) nij[c] = (long long)t[c] + t[9 + c];
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 3; ++i) {
            nik[3 * k + i] = (long long)t[9 * k + 3 * i] + t[9 * k + 3 * i + 1] + t[9 * k + 3 * i + 2];
            njk[3 * k + i] = (long long)t[9 * k + i] + t[9 * k + 3 + i] + t[9 * k + 6 + i]; // (here i is the code j)
        }
    for (int i = 0; i < 3; ++i) {
        ni[i] = nik[i] + nik[3 + i];
        nj[i] = njk[i] + njk[3 + i];
    }
    for (int k = 0; k < 2; ++k) nk[k] = nik[3 * k] + nik[3 * k + 1] + nik[3 * k + 2];
    n = nk[0] + nk[1];
    double q[18], eta = 0.0;
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const int c = 9 * k + 3 * i + j;
                const bool live = ni[i] > 0 && nj[j] > 0 && nk[k] > 0;
                q[c] = live ? (((double)nij[3 * i + j] * (double)nik[3 * k + i]) * (double)njk[3 * k + j]) / (((double)ni[i] * (double)nj[j]) * (double)nk[k]) : 0.0;
                eta += q[c];
            }
    double s = 0.0, a = 0.0;
    for (int c = 0; c < 18; ++c) {
        if (t[c] <= 0) continue;
        const double x = (double)t[c], ls = log(x / (double)n), lk = log(q[c] / eta);
        s += x * (ls - lk);
        a += x * (fabs(ls) + fabs(lk));
    }
    if (abs_terms) *abs_terms = a;
    return 2.0 * s;
}

// The slack of the screen as a function of the rows n >= 2 a table can hold: 2^-44 times the bound
// 2 n (4 ln n + ln 18) of the sum of the absolute terms
HG_EPI_HD inline double hg_epi_delta(double n)
{
    if (n < 2.0) n = 2.0;
    return 5.6843418860808015e-14 * (2.0 * n * (4.0 * log(n) + 2.8903717578961645));
}
