// hg_hefit.cpp -- Haseman-Elston regression from the row sums of hgibbs_grm_rowsums: plain C++, no HIP.
//
// Over all m = n'(n' - 1)/2 pairs a < b of the used rows, regress z_ab on A_ab by OLS with an intercept, for z = y_a y_b (HE-CP) and
// z = (y_a - y_b)^2 (HE-SD).  The fit needs five sums over the pairs; with p_k = sum y^k over the used rows and the row sums
// a1_a = sum_b A_ab, a2_a = sum_b A_ab^2, ay_a = sum_b A_ab y_b, ayy_a = sum_b A_ab y_b^2 (b over the partners of a) they are
//
//     sum A = 1/2 sum a1        sum A^2 = 1/2 sum a2
//     CP:  sum z = (p1^2 - p2)/2       sum A z = 1/2 sum y_a ay_a                  sum z^2 = (p2^2 - p4)/2
//     SD:  sum z = n' p2 - p1^2        sum A z = sum y_a^2 a1_a - sum y_a ay_a     sum z^2 = n' p4 - 4 p1 p3 + 3 p2^2
//
// and taking individual a's n' - 1 pairs out of them is closed form too (he_fit below), so the delete-one-individual jackknife costs
// O(n') on the host and nothing on the device.  The sums run in long double: the inputs are f64 and n' of them cost nothing here.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/hgibbs.h"

extern "C" void hgibbs_set_error_(const char* msg);

namespace {

typedef long double ld;

int hfail(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    hgibbs_set_error_(buf);
    return 1;
}

// the five sums of one regression over m pairs
struct Sums {
    ld m, A, AA, z, Az;
};

// slope and intercept; false when A is constant over the pairs
bool ols(const Sums& s, ld& slope, ld& icpt, ld& den)
{
    den = s.m * s.AA - s.A * s.A;
    if (!(den > 0.0L)) return false;
    slope = (s.m * s.Az - s.A * s.z) / den;
    icpt = (s.z - slope * s.A) / s.m;
    return true;
}

double p_normal(ld est, ld se) { return (double)std::erfc((double)(std::fabs(est / se) / std::sqrt(2.0L))); }

} // namespace

extern "C" int hgibbs_he_fit(uint32_t n, const double* y, const double* ay, const double* ayy, const double* a1, const double* a2,
                             const uint32_t* partners, hgibbs_he_result* out)
{
    if (!y || !ay || !ayy || !a1 || !a2 || !partners || !out) return hfail("hgibbs_he_fit: null argument");
    std::vector<uint32_t> rows;
    for (uint32_t a = 0; a < n; ++a)
        if (partners[a]) rows.push_back(a);
    const uint32_t nu = (uint32_t)rows.size();
    if (nu < 4u) return hfail("hgibbs_he_fit: %u rows with a partner, the regression and its jackknife need at least 4", nu);
    for (uint32_t a : rows) {
        if (partners[a] != nu - 1u)
            return hfail("hgibbs_he_fit: row %u has %u partners where the %u rows with a partner should each have %u: the closed forms need "
                         "every pair of the used rows", a, partners[a], nu, nu - 1u);
        if (!std::isfinite(y[a]) || !std::isfinite(ay[a]) || !std::isfinite(ayy[a]) || !std::isfinite(a1[a]) || !std::isfinite(a2[a]))
            return hfail("hgibbs_he_fit: a non-finite input at row %u", a);
    }

    const ld np = nu;
    ld p1 = 0, p2 = 0, p3 = 0, p4 = 0, s1 = 0, s2 = 0, syay = 0, syya1 = 0;
    for (uint32_t a : rows) {
        const ld v = y[a];
        p1 += v;
        p2 += v * v;
        p3 += v * v * v;
        p4 += v * v * v * v;
        s1 += a1[a];
        s2 += a2[a];
        syay += v * (ld)ay[a];
        syya1 += v * v * (ld)a1[a];
    }
    const ld m = np * (np - 1) / 2;
    const Sums full[2] = {{m, s1 / 2, s2 / 2, (p1 * p1 - p2) / 2, syay / 2}, {m, s1 / 2, s2 / 2, np * p2 - p1 * p1, syya1 - syay}};
    const ld zz[2] = {(p2 * p2 - p4) / 2, np * p4 - 4 * p1 * p3 + 3 * p2 * p2};
    const ld mean = p1 / np;
    ld vp = 0;
    for (uint32_t a : rows) vp += ((ld)y[a] - mean) * ((ld)y[a] - mean);
    vp /= np - 1;
    if (!(vp > 0.0L)) return hfail("hgibbs_he_fit: y is constant over the %u used rows (Vp = 0)", nu);

    hgibbs_he_result res{};
    res.n_used = nu;
    res.n_left_out = n - nu;
    res.pairs = (uint64_t)nu * (nu - 1u) / 2u;
    res.vp = (double)vp;
    std::vector<ld> js(nu), ji(nu);
    for (int f = 0; f < 2; ++f) {
        ld slope, icpt, den;
        if (!ols(full[f], slope, icpt, den))
            return hfail("hgibbs_he_fit: A is constant over the %llu pairs (m sum A^2 - (sum A)^2 <= 0): no slope", (unsigned long long)res.pairs);
        const ld rss = zz[f] - icpt * full[f].z - slope * full[f].Az;
        const ld s2e = rss / (m - 2);
        const ld se_s = std::sqrt(s2e * m / den), se_i = std::sqrt(s2e * full[f].AA / den);
        // delete one individual: its n' - 1 pairs leave every sum
        ld ms = 0, mi = 0;
        for (uint32_t x = 0; x < nu; ++x) {
            const uint32_t a = rows[x];
            const ld v = y[a];
            Sums d = full[f];
            d.m -= np - 1;
            d.A -= a1[a];
            d.AA -= a2[a];
            if (f == 0) {
                d.z -= v * (p1 - v);
                d.Az -= v * (ld)ay[a];
            } else {
                d.z -= np * v * v - 2 * v * p1 + p2;
                d.Az -= v * v * (ld)a1[a] - 2 * v * (ld)ay[a] + (ld)ayy[a];
            }
            ld dd;
            if (!ols(d, js[x], ji[x], dd)) return hfail("hgibbs_he_fit: A is constant over the pairs that remain without row %u: no jackknife", a);
            ms += js[x];
            mi += ji[x];
        }
        ms /= np;
        mi /= np;
        ld vs = 0, vi = 0;
        for (uint32_t x = 0; x < nu; ++x) {
            vs += (js[x] - ms) * (js[x] - ms);
            vi += (ji[x] - mi) * (ji[x] - mi);
        }
        const ld jk_s = std::sqrt((np - 1) / np * vs), jk_i = std::sqrt((np - 1) / np * vi);
        const ld k = f == 0 ? 1 / vp : -1 / (2 * vp); // h2 = slope / Vp (CP), -slope / (2 Vp) (SD): Vp taken as fixed
        hgibbs_he_form& o = f == 0 ? res.cp : res.sd;
        o.intercept = (double)icpt;
        o.slope = (double)slope;
        o.h2 = (double)(k * slope);
        o.intercept_se = (double)se_i;
        o.slope_se = (double)se_s;
        o.h2_se = (double)(std::fabs(k) * se_s);
        o.intercept_se_jk = (double)jk_i;
        o.slope_se_jk = (double)jk_s;
        o.h2_se_jk = (double)(std::fabs(k) * jk_s);
        o.intercept_p = p_normal(icpt, se_i);
        o.slope_p = p_normal(slope, se_s);
        o.intercept_p_jk = p_normal(icpt, jk_i);
        o.slope_p_jk = p_normal(slope, jk_s);
    }
    *out = res;
    return 0;
}
