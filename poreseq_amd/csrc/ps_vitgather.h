// ps_vitgather.h — the host walk of ViterbiMutate over the reference positions (cpp/Viterbi.cpp:261-325): which positions are kept
// and the mean level per (position, event).  Pure host index arithmetic on plain arrays, without a dependency: ps_vit.cpp fills the
// view from an AlignData and its JobOut records, tests/native/vitgather_check.cpp from crafted arrays, under a sanitizer.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ps {

// One AlignData as the walk reads it: per event its level count, where its levels start in the four arrays (all events
// concatenated), and what updaterefs left of its ref_index (has_index false: empty, getrefstates finds nothing)
struct VitGatherEvent { int n; int64_t off; bool has_index; int refstart, refend; };
struct VitGatherIn {
    int E;
    const VitGatherEvent* ev;                             // [E]
    const double *ref_align, *ref_index, *mean, *stdv;    // [levels of all events]
};
// obsin[T][E][4] = {level mean, sd mean, log(sd mean), present} of the T kept positions
struct VitGather { std::vector<double> obsin; int T = 0; };

inline void vit_gather(const VitGatherIn& in, VitGather* g) {
    const int E = in.E;
    // first level whose ref_index equals an integer position (std::find in getrefstates, cpp/EventData.h:192),
    // as a flat table per event indexed by position + 1 (positions outside [-1, maxpos] never match)
    // (extrapolated ref_index values past refend can be integers too and do take part, so the table
    // spans every integer-valued entry).  The table starts at position -1: a read without an aligned level has refstart = -1, the
    // walk then begins there, and std::find meets the -1 markers that an un-interpolated hole keeps (behind an aligned level 0,
    // cpp/EventData.h:157) or a head that the line through the end levels crosses at -1; no position lies below -1.
    int maxpos = 0;
    for (int e = 0; e < E; e++) {
        if (!in.ev[e].has_index) continue;
        const double* ri = in.ref_index + in.ev[e].off;
        for (int t = 0; t < in.ev[e].n; t++) {
            const double v = ri[t];
            if (v >= 0.0 && v < 1e9 && v == std::floor(v)) maxpos = std::max(maxpos, (int)v);
        }
    }
    std::vector<std::vector<int>> first(E);
    for (int e = 0; e < E; e++) {
        if (!in.ev[e].has_index) continue;  // empty ref_index: getrefstates finds nothing
        first[e].assign((size_t)maxpos + 2, -1);
        const double* ri = in.ref_index + in.ev[e].off;
        for (int t = 0; t < in.ev[e].n; t++) {
            const double v = ri[t];
            if (v >= -1.0 && v <= (double)maxpos && v == std::floor(v)) {
                int& slot = first[e][(size_t)((int)v + 1)];
                if (slot < 0) slot = t;
            }
        }
    }
    auto rstart = [&](int e) { return in.ev[e].has_index ? in.ev[e].refstart : -1; };
    auto rend = [&](int e) { return in.ev[e].has_index ? in.ev[e].refend : -1; };
    int refind = rstart(0);
    for (int e = 0; e < E; e++) refind = std::min(refind, rstart(e));
    std::vector<double>& obsin = g->obsin;
    int T = 0;
    while (true) {
        int nl = 0, nal = 0;
        const size_t at = obsin.size();
        obsin.resize(at + (size_t)E * 4, 0.0);
        for (int e = 0; e < E; e++) {
            if (refind < -1 || refind > maxpos || first[e].empty() || first[e][refind + 1] < 0) continue;
            const double* ra = in.ref_align + in.ev[e].off;
            const double* mean = in.mean + in.ev[e].off;
            const double* stdv = in.stdv + in.ev[e].off;
            int t = first[e][refind + 1], cnt = 1;
            // getrefstates keeps following levels while ref_align <= refind, using those > 0 (cpp/EventData.h:197-201)
            double lsum = 0, ssum = 0;
            lsum += mean[t]; ssum += stdv[t];
            for (t++; t < in.ev[e].n && ra[t] <= refind; t++)
                if (ra[t] > 0) { lsum += mean[t]; ssum += stdv[t]; cnt++; }
            const double lvl = lsum / cnt, sd = ssum / cnt;
            nl++;
            double* o = obsin.data() + at + (size_t)e * 4;
            o[0] = lvl; o[1] = sd; o[2] = std::log(sd); o[3] = 1.0;
        }
        for (int e = 0; e < E; e++) if (refind >= rstart(e) && refind <= rend(e)) nal++;
        if (nl <= nal * 0.2) {
            obsin.resize(at);
            if (nal == 0) break;
            refind++;
            continue;
        }
        T++;
        refind++;
    }
    g->T = T;
}

}  // namespace ps
