// emission_check.cpp — test program (tests/test_edge_values.py): the emission log-density of ps_dev.h (emission8) restated in plain
// C++ both ways — quotients by Markstein's sequence on tabulated reciprocals y = RN(1/b), and by IEEE division — over a grid of
// everything the host's predicate (poreseq_amd/csrc/ps_sane.h, the same header ps_align.cpp decides with) accepts: each divisor
// from just inside the lower bound to just inside the upper, numerators that make a1, a2 and t zero, subnormal, about 1, 1e150, 1e200
// and overflowing, lambda from 0 to past its bound.  For every ACCEPTED tuple the two must have identical bits, or both be NaN.
// Prints the counts; exit status 1 on any mismatch.  `emission_check old` evaluates the predicate the library had before
// (finite divisors in (1e-100, 1e100), |mean| and |lambda| <= 1e100) and shows where that one failed.
// Build with -ffp-contract=off -mfma (the compiler must neither fuse nor split an operation).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../poreseq_amd/csrc/ps_sane.h"

static inline double mdiv(double a, double b, double y) {
    double q = a * y;
    double r = std::fma(-b, q, a);
    q = std::fma(r, y, q);
    r = std::fma(-b, q, a);
    return std::fma(r, y, q);
}

// m = {mu, 1/sg, sg, log sg, sm, 1/sm, lambda, log lambda}; lev = {x, sd, 3 log sd(mirrored level), 1/sd}
template <bool FASTDIV>
static double emission8(const double (&m)[8], const double (&lev)[4], const double log2pi, const double off) {
    const double a1 = lev[0] - m[0], a2 = lev[1] - m[4];
    const double d = FASTDIV ? mdiv(a1, m[2], m[1]) : a1 / m[2];
    const double e = FASTDIV ? mdiv(a2, m[4], m[5]) : a2 / m[4];
    double l = -0.5 * (d * d + log2pi) - m[3];
    const double t = e * e * m[6];
    const double q = FASTDIV ? mdiv(t, lev[1], lev[3]) : t / lev[1];
    const double g = 0.5 * (m[7] - lev[2] - log2pi - q);
    l += g;
    l += off;
    return l;
}

static bool old_sane(double v) { return std::isfinite(v) && v > 1e-100 && v < 1e100; }
static bool old_accepts(double x, double sd, double mu, double sg, double sm, double lam) {
    return old_sane(sg) && old_sane(sm) && std::isfinite(mu) && std::isfinite(lam) && std::fabs(mu) <= 1e100 && std::fabs(lam) <= 1e100 &&
           old_sane(sd) && std::isfinite(x) && std::fabs(x) <= 1e100;
}

static void add_unique(std::vector<double>& v, double x) {
    for (double y : v) if (!std::memcmp(&x, &y, 8)) return;
    v.push_back(x);
}

int main(int argc, char** argv) {
    const bool old = argc > 1 && !std::strcmp(argv[1], "old");
    const double lo = old ? 1e-100 : ps::SANE_LO, hi = old ? 1e100 : ps::SANE_HI;
    const double inf = INFINITY;
    // divisors: the ends of the range, one step inside and one step outside (the predicate must cut there), the decades between
    std::vector<double> div;
    for (double v : {std::nextafter(lo, 0.0), lo, std::nextafter(lo, inf), 1e-60, 1e-30, 0.75, 1.0, 1.0 + 0x1p-52, 3.0, 1e30, 1e60,
                     std::nextafter(hi, 0.0), hi, std::nextafter(hi, inf)})
        add_unique(div, v);
    const double lam_hi = old ? 1e100 : ps::SANE_LAM_HI, lam_lo = old ? 0.0 : ps::SANE_LAM_LO;
    std::vector<double> lams;
    for (double v : {0.0, 4.9e-324, 1e-310, std::nextafter(lam_lo, 0.0), lam_lo, std::nextafter(lam_lo, inf), 1e-30, 1.0, 40.0, 1e30,
                     std::nextafter(lam_hi, 0.0), lam_hi, std::nextafter(lam_hi, inf)})
        add_unique(lams, v);
    // numerator targets: a1 = x - mu and a2 = sd - sm are reached by choosing x (any mean) and sd (a divisor) around mu and sm
    const double mags[] = {0.0, 4.9e-324, 1e-310, 2.3e-308, 1e-200, 1e-150, 1e-30, 0x1p-52, 1.0, 65.0, 1e30, 1e150, 1e200, 1e300, 1.7e308};
    std::vector<double> mus;
    for (double v : {0.0, -0.0, 4.9e-324, 1e-310, lo, -lo, std::nextafter(lo, 0.0), 1.0, -65.0, 1e30, hi, -hi, std::nextafter(hi, inf)})
        add_unique(mus, v);
    const double log2pi = std::log(2 * M_PI), off = 4.5;
    long n = 0, accepted = 0, bad = 0, nonfinite = 0;
    for (double sg : div) for (double sm : div) for (double lam : lams) for (double mu : mus) {
        // candidate level means: mu +- each magnitude, and the magnitudes themselves
        std::vector<double> xs;
        for (double a : mags) { add_unique(xs, mu + a); add_unique(xs, mu - a); add_unique(xs, a); add_unique(xs, -a); }
        add_unique(xs, std::nextafter(mu, inf)); add_unique(xs, std::nextafter(mu, -inf));
        // candidate level stdvs: every grid divisor, sm's neighbours (a2 of one ulp), sm +- each magnitude where that is a number
        std::vector<double> sds = div;
        add_unique(sds, sm); add_unique(sds, std::nextafter(sm, inf)); add_unique(sds, std::nextafter(sm, 0.0));
        for (double a : mags) { add_unique(sds, sm + a); if (sm - a > 0) add_unique(sds, sm - a); }
        for (double sd : sds) {
            // the level whose log stdv the row reads is the mirrored one: any accepted divisor; its ends and 1 are enough (one addend)
            for (double sdm : {lo, 1.0, hi}) for (double x : xs) {
                n++;
                const bool ok = old ? old_accepts(x, sd, mu, sg, sm, lam)
                                    : ps::sane_model_row(mu, sg, sm, lam) && ps::sane_level(x, sd) && ps::sane_level(0.0, sdm);
                if (!ok) continue;
                accepted++;
                const double m[8] = {mu, 1.0 / sg, sg, std::log(sg), sm, 1.0 / sm, lam, std::log(lam)};
                const double lev[4] = {x, sd, 3 * std::log(sdm), 1.0 / sd};
                const double f = emission8<true>(m, lev, log2pi, off), g = emission8<false>(m, lev, log2pi, off);
                if (!std::isfinite(g)) nonfinite++;
                if (std::memcmp(&f, &g, 8) && !(std::isnan(f) && std::isnan(g))) {
                    if (bad++ < 8) std::printf("mismatch x=%a sd=%a mu=%a sg=%a sm=%a lam=%a: fast %a ieee %a\n", x, sd, mu, sg, sm, lam, f, g);
                }
            }
        }
    }
    // random significands at the extreme and middle binades of the accepted range (the grid above is mostly powers of two and short
    // decimals): every tuple drawn is accepted by construction, which the predicate must confirm
    long drawn = 0;
    if (!old) {
        uint64_t rng = 88172645463325252ull;
        auto xs64 = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
        auto draw = [&](const int* ex, int nex, bool any_sign, bool may_be_zero) {
            const uint64_t r = xs64();
            if (may_be_zero && r % 16 == 0) return 0.0;
            const int e = ex[(r >> 8) % nex];
            const uint64_t mant = (r % 7 == 0) ? 0ull : (r % 7 == 1) ? 0x000fffffffffffffull : (xs64() & 0x000fffffffffffffull);
            const uint64_t u = ((uint64_t)(1023 + e) << 52) | mant | ((any_sign && (r >> 40 & 1)) ? 0x8000000000000000ull : 0ull);
            double v; std::memcpy(&v, &u, 8);
            return v;
        };
        const int dex[] = {-128, -127, -64, -1, 0, 1, 6, 64, 126, 127}, lex[] = {-200, -199, -100, -1, 0, 5, 100, 198, 199};
        for (long k = 0; k < 4000000; k++) {
            const double sg = draw(dex, 10, false, false), sm = draw(dex, 10, false, false), sdm = draw(dex, 10, false, false);
            const double sd = (k & 3) == 0 ? std::nextafter(sm, (k & 4) ? 0.0 : inf) : draw(dex, 10, false, false);
            const double mu = draw(dex, 10, true, true), lam = draw(lex, 9, false, false);
            const double x = (k & 24) == 0 ? std::nextafter(mu, (k & 32) ? -inf : inf) : draw(dex, 10, true, true);
            if (!(ps::sane_model_row(mu, sg, sm, lam) && ps::sane_level(x, sd) && ps::sane_level(0.0, sdm))) continue;   // (a neighbour one step outside)
            drawn++;
            const double m[8] = {mu, 1.0 / sg, sg, std::log(sg), sm, 1.0 / sm, lam, std::log(lam)};
            const double lev[4] = {x, sd, 3 * std::log(sdm), 1.0 / sd};
            const double f = emission8<true>(m, lev, log2pi, off), g = emission8<false>(m, lev, log2pi, off);
            if (!std::isfinite(g)) nonfinite++;
            if (std::memcmp(&f, &g, 8)) {
                if (bad++ < 8) std::printf("mismatch x=%a sd=%a mu=%a sg=%a sm=%a lam=%a: fast %a ieee %a\n", x, sd, mu, sg, sm, lam, f, g);
            }
        }
        accepted += drawn;
    }
    std::printf("predicate=%s tuples=%ld accepted=%ld nonfinite=%ld mismatches=%ld\n", old ? "old" : "ps_sane.h", n, accepted, nonfinite, bad);
    return bad ? 1 : 0;
}
