// ps_sane.h — which event and model tables may take the tabulated-reciprocal (Markstein) build of the emission: pure, host-only, no
// HIP include.  Shared by the library (ps_align.cpp decides with it at ps_align_create) and by a host test of it
// (tests/native/emission_check.cpp), which evaluates both builds of the emission over the corners of what is accepted here.
//
// The range (DESIGN.md section 2 derives it).  With a = the numerator, b = the divisor and y = RN(1/b), the sequence
//   q0 = a*y; r = fma(-b,q0,a); q1 = fma(r,y,q0); r = fma(-b,q1,a); q = fma(r,y,q1)
// is RN(a/b) when b and y are normal, a is zero or at least 2^-960 in magnitude (both residuals are then exact) and a/b is a normal
// number far from overflow.  An emission (ps_dev.h, emission8) forms
//   d = (x - mu) / sg        e = (sd - sm) / sm        q = e*e*lam / sd
// from a level {x, sd} and a model row {mu, sg, sm, lam = sm^3 / ss^2}.  Accepted:
//   divisors   sg, sm, sd        in [2^-128, 2^128]
//   means      x, mu             zero, or of magnitude in [2^-128, 2^128]
//   lambda                       in [2^-200, 2^200]   (the only way ss enters; excludes ss = 0, infinite, NaN and the underflow to 0)
// Every accepted number is a multiple of 2^-180, so a difference of two is zero or at least 2^-180 and at most 2^129:
//   |d|, |e| in [2^-308, 2^257],  d*d, e*e in [2^-616, 2^514],  t = e*e*lam in [2^-816, 2^714],  q in [2^-944, 2^842]
// — no numerator below 2^-960, no quotient or product subnormal, infinite or NaN.  Anything else takes the IEEE-division build.
#pragma once
#include <cmath>
#include <cstdint>

namespace ps {

constexpr double SANE_LO = 0x1p-128, SANE_HI = 0x1p128;          // divisors; magnitudes of non-zero means
constexpr double SANE_LAM_LO = 0x1p-200, SANE_LAM_HI = 0x1p200;  // lambda = sd_mean^3 / sd_stdv^2

inline bool sane_divisor(double v) { return v >= SANE_LO && v <= SANE_HI; }                                 // (false for NaN)
inline bool sane_mean(double v) { const double a = std::fabs(v); return a == 0.0 || (a >= SANE_LO && a <= SANE_HI); }
inline bool sane_lambda(double v) { return v >= SANE_LAM_LO && v <= SANE_LAM_HI; }

// lambda of a model row as the host tables hold it (ModelData::setData, cpp/EventData.h:48-73)
inline double model_lambda(double sd_mean, double sd_stdv) { return std::pow(sd_mean, 3) / std::pow(sd_stdv, 2); }

// one model row: level mean, level stdv, sd mean and lambda as the device tables hold them
inline bool sane_model_row(double level_mean, double level_stdv, double sd_mean, double lambda) {
    return sane_mean(level_mean) && sane_divisor(level_stdv) && sane_divisor(sd_mean) && sane_lambda(lambda);
}
// one level of an event
inline bool sane_level(double mean, double stdv) { return sane_mean(mean) && sane_divisor(stdv); }

// ---- values that make an emission infinite or NaN --------------------------------------------------------
// An emission is  -0.5 (d d + log 2 pi) - log sg + 0.5 (log lambda - 3 log sd' - log 2 pi - e e lambda / sd) + lik_offset  with sd' the
// mirrored level's stdv.  It can be +infinity only through  log sg = -inf (sg == 0),  log lambda = +inf,  log sd' = -inf (a level
// with stdv == 0)  or an infinite lik_offset.  A +infinity emission is what the kernels cannot take: "no cell" is the FINITE value
// -1.797e308 there (keep_or_absent, ps_dev.h), which loses every maximum only as long as nothing infinite is added to it.  Such
// tables are refused by ps_align_create.
inline bool level_plus_inf(double stdv) { return stdv == 0.0; }
inline bool model_row_plus_inf(double level_stdv, double lambda) { return level_stdv == 0.0 || (std::isinf(lambda) && lambda > 0); }
inline bool offset_refused(double lik_offset) { return !std::isfinite(lik_offset); }
// Everything else outside the reference's domain gives emissions that are finite, -infinity or NaN — candidates that never win a
// maximum, in the reference (`if (lik > cur)`) and in the kernels (v_max_f64 drops a NaN operand): the dynamic programming and
// the edit scoring run on them.  ViterbiMutate does not (a position whose emissions are all NaN leaves no back-pointer): an
// AlignData that holds one of these is marked, and that call refuses it.
inline bool level_nonfinite(double mean, double stdv) { return !std::isfinite(mean) || !std::isfinite(stdv) || !(stdv > 0.0); }
inline bool model_row_nonfinite(double level_mean, double level_stdv, double sd_mean, double lambda) {
    return !std::isfinite(level_mean) || !(std::isfinite(level_stdv) && level_stdv > 0.0) || !(std::isfinite(sd_mean) && sd_mean > 0.0) ||
           !(std::isfinite(lambda) && lambda > 0.0);
}

}  // namespace ps
