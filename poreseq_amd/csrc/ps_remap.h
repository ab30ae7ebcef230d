// ps_remap.h — PSEvent.mapaligns (poreseq/EventData.py:226-256) restated for Smith-Waterman index lists; host and device, no HIP headers
// (tests/native/remap_check.cpp compiles this text with g++ and compares it with the Python rule).
//
// mapaligns makes the pairs unique in the first index (np.unique: sorted, the first entry of each value), then
//   ref_align[ref_align > 0] = np.round(np.interp(ref_align, inds1, inds2, left = 0, right = 0)).
// In swfull's lists (cpp/swlib.cpp:279-333) every seq1 index between the lowest non-zero one (lo) and the highest (hi) occurs exactly
// once, with its partner or 0 where the base faces a gap; all entries with inds1 == 0 (bases only seq2 has) collapse to ONE
// interpolation point (0, y0), y0 = inds2 of the first of them in list order.  So the x grid is [0,] lo, lo + 1, ..., hi and the
// lookup is a table read — except below lo, where numpy interpolates between (0, y0) and (lo, part[lo]) when the lists hold such an
// entry (a variant clipped on the left that carries an insertion: every level left of the alignment lands on a slanted line).
#ifndef PS_REMAP_H_
#define PS_REMAP_H_

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PS_REMAP_HD __host__ __device__
#else
#define PS_REMAP_HD
#endif

namespace ps {

// what the SW_MAP traceback leaves per pair besides the partner table: lo / hi = lowest / highest non-zero seq1 index of the lists,
// has0 = the lists hold an entry with inds1 == 0, y0 = inds2 of the first such entry in list order
struct RemapRec { int lo, hi, has0, y0; };

// new ref_align of a level whose old one is x; part[i1] = i2 (0: gap) for lo <= i1 <= hi.  The arithmetic is numpy's
// (npy_interp: slope = dy / dx by IEEE division, slope * (x - x_j) + y_j as a separate multiply and add — build with
// -ffp-contract=off — and np.round = rint, half to even).
PS_REMAP_HD inline double remap_level(double x, const int* part, RemapRec r) {
    if (!(x > 0)) return 0.0;                       // ref_align <= 0 (and NaN) stays cleared
    if (r.hi <= 0 || x > (double)r.hi) return 0.0;  // right of the last point
    if (x < (double)r.lo) {
        if (!r.has0) return 0.0;                    // left of the first point
        const double slope = ((double)part[r.lo] - (double)r.y0) / ((double)r.lo - 0.0);
        return rint(slope * (x - 0.0) + (double)r.y0);
    }
    const double fl = floor(x);
    const int j = (int)fl;
    if (x == fl) return (double)part[j];            // on a grid point (ref_align holds integers: the only case the drivers produce)
    const double slope = ((double)part[j + 1] - (double)part[j]) / ((fl + 1.0) - fl);
    return rint(slope * (x - fl) + (double)part[j]);
}

}  // namespace ps
#endif
