// Host check of ViterbiMutate's walk over the reference positions (poreseq_amd/csrc/ps_vitgather.h), meant to be built with
// -fsanitize=address,undefined: ref_align, ref_index, mean, stdv and the event records are heap blocks of exactly their own size
// (the events concatenated, as in an AlignData), so a table index or a level index outside its array reads outside the block or
// lands in a neighbour's levels, which the comparison catches.
//
// T and every obsin record are compared, by bytes, with a naive restatement of cpp/Viterbi.cpp:261-325 and cpp/EventData.h:186-204
// written here: per position and event a linear search of ref_index for equality, the follow-on levels while ref_align <= position
// (those > 0 count), then the one-fifth skip rule and the stop rule.
//
// Crafted: a read without an aligned level (the walk starts at -1); -1 markers kept in ref_index behind an aligned level 0; whole
// ref_index values past the largest refend (positions the draft does not have); a position one of six reads covers (skipped); a gap
// no read spans (the walk stops); an event of 0 levels; E = 1; an event whose has_index is false over misleading arrays;
// fractional and NaN ref_index; values at and above 1e9, infinities and values below -1, which the table must ignore.
// Random: seeded compositions of the same families, fewer than 300 levels per event.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../poreseq_amd/csrc/ps_vitgather.h"

static long bad = 0, checks = 0;
static unsigned long long rs = 88172645463325252ull;
static int rnd(int n) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (int)(rs % (unsigned long long)n); }
static double urnd() { return rnd(1 << 20) / (double)(1 << 20); }

#define EXPECT(c)                                                        \
    do {                                                                 \
        checks++;                                                        \
        if (!(c)) { bad++; printf("FAIL line %d: %s\n", __LINE__, #c); } \
    } while (0)

struct Ev {
    std::vector<double> ra, ri, mean, stdv;
    bool has_index = false;
    int refstart = -1, refend = -1;
    int n() const { return (int)ra.size(); }
    void level(double a, double i) { ra.push_back(a); ri.push_back(i); mean.push_back(40.0 + 60.0 * urnd()); stdv.push_back(0.3 + 2.0 * urnd()); }
    // updaterefs' span of the aligned levels (cpp/EventData.h:135-136); ref_index stays what the case wrote
    void span() {
        has_index = false; refstart = refend = -1;
        for (int t = 0; t < n(); t++)
            if (ra[t] > 0) { if (!has_index) refstart = (int)ra[t]; refend = (int)ra[t]; has_index = true; }
    }
};
typedef std::vector<Ev> Case;

// ---- families.  A plain read: aligned levels from `from`, with stays (a column twice) and skips (a column left out), covering
// at least up to `to`
static Ev plain(int from, int to, int max_levels = 290) {
    Ev e;
    for (int c = from; c <= to && e.n() < max_levels; ) {
        e.level(c, c);
        const int r = rnd(10);
        c += r == 0 ? 0 : r == 1 ? 2 : 1;
    }
    e.span();
    return e;
}
// a level in (0, 1) in front: aligned, column 0 (refstart = 0), so that a walk that started at -1 does not stop at position 0
static Ev col0(Ev e) {
    Ev f;
    f.level(0.5, 0.5);
    for (int t = 0; t < e.n(); t++) { f.ra.push_back(e.ra[t]); f.ri.push_back(e.ri[t]); f.mean.push_back(e.mean[t]); f.stdv.push_back(e.stdv[t]); }
    f.span();
    return f;
}
static Ev unaligned(int n) {   // no aligned level: markers only, ref_index empty
    Ev e;
    const double marks[] = {0.0, -1.0, std::nan("")};
    for (int t = 0; t < n; t++) { const double m = marks[rnd(3)]; e.level(m, m); }
    e.span();
    return e;
}
static Ev markers_behind_level0(int from, int to) {   // level 0 aligned, an un-interpolated hole of -1 / 0 / NaN behind it
    Ev e = plain(from, to, 250);
    Ev f;
    f.level(from, from);
    const double marks[] = {-1.0, 0.0, -1.0, std::nan(""), -1.0};
    const int h = 1 + rnd(5);
    for (int k = 0; k < h; k++) f.level(marks[k], marks[k]);
    for (int t = 0; t < e.n(); t++) { f.ra.push_back(e.ra[t]); f.ri.push_back(e.ri[t]); f.mean.push_back(e.mean[t]); f.stdv.push_back(e.stdv[t]); }
    f.span();
    return f;
}
static Ev overhang(int from, int to, int extra) {   // unaligned tail whose extrapolated ref_index are whole numbers past refend
    Ev e = plain(from, to, 250);
    const int last = e.refend;
    for (int k = 1; k <= extra; k++) e.level(0.0, last + k);
    e.span();
    return e;
}
static Ev holes(int from, int to) {   // interpolated holes: fractional, whole and NaN ref_index on unaligned levels; aligned fractions
    Ev e = plain(from, to, 280);
    for (int t = 1; t + 1 < e.n(); t++) {
        const int r = rnd(12);
        if (r == 0) { e.ra[t] = 0.0; e.ri[t] = e.ri[t - 1] + 0.5; }
        else if (r == 1) { e.ra[t] = -1.0; e.ri[t] = std::nan(""); }
        else if (r == 2) { e.ra[t] = 0.0; e.ri[t] = std::floor(e.ri[t - 1]) + 1.0; }   // a whole number on an unaligned level
        else if (r == 3) { e.ra[t] += 0.25; e.ri[t] = e.ra[t]; }                        // aligned, between two columns
    }
    e.span();
    return e;
}
static Ev huge(int from, int to) {   // head and tail entries the table must ignore
    Ev e;
    const double head[] = {-2.0, -5.5, -INFINITY, -1e300};
    for (int k = 0, h = rnd(5); k < h; k++) e.level(0.0, head[k]);
    Ev p = plain(from, to, 250);
    for (int t = 0; t < p.n(); t++) { e.ra.push_back(p.ra[t]); e.ri.push_back(p.ri[t]); e.mean.push_back(p.mean[t]); e.stdv.push_back(p.stdv[t]); }
    const double tail[] = {1e9, 1e9 + 1, 3e9, 4294967296.0, 1e300, INFINITY, 999999999.5};
    for (int k = 0, h = 1 + rnd(7); k < h; k++) e.level(0.0, tail[k]);
    e.span();
    return e;
}
static Ev no_index_over_arrays(int from, int to) {   // has_index false: the arrays and the span must not be looked at
    Ev e = plain(from, to, 200);
    e.has_index = false;
    return e;
}

// ---- the naive restatement
struct Want { int T = 0; std::vector<double> obsin; };
static Want naive(const Case& c) {
    const int E = (int)c.size();
    auto rstart = [&](int e) { return c[e].has_index ? c[e].refstart : -1; };
    auto rend = [&](int e) { return c[e].has_index ? c[e].refend : -1; };
    int refind = rstart(0);
    for (int e = 0; e < E; e++) if (rstart(e) < refind) refind = rstart(e);
    Want w;
    for (long guard = 0;; guard++) {
        if (guard > 1000000) { printf("naive: the walk does not stop\n"); exit(2); }
        std::vector<double> rec((size_t)E * 4, 0.0);
        int nl = 0, nal = 0;
        for (int e = 0; e < E; e++) {
            const Ev& v = c[e];
            if (!v.has_index) continue;
            int t = 0;
            while (t < v.n() && !(v.ri.at(t) == (double)refind)) t++;
            if (t == v.n()) continue;
            double lsum = v.mean.at(t), ssum = v.stdv.at(t);
            int cnt = 1;
            for (t++; t < v.n() && v.ra.at(t) <= refind; t++)
                if (v.ra.at(t) > 0) { lsum += v.mean.at(t); ssum += v.stdv.at(t); cnt++; }
            const double sd = ssum / cnt;
            rec[(size_t)e * 4 + 0] = lsum / cnt; rec[(size_t)e * 4 + 1] = sd; rec[(size_t)e * 4 + 2] = std::log(sd); rec[(size_t)e * 4 + 3] = 1.0;
            nl++;
        }
        for (int e = 0; e < E; e++) if (refind >= rstart(e) && refind <= rend(e)) nal++;
        if (nl <= nal * 0.2) {
            if (nal == 0) break;
            refind++;
            continue;
        }
        w.obsin.insert(w.obsin.end(), rec.begin(), rec.end());
        w.T++;
        refind++;
    }
    return w;
}

template <class T> static T* heap(size_t n) { return (T*)malloc(n ? n * sizeof(T) : 1); }

// the library's walk on heap blocks of exactly the case's size; returns T (for the families' own expectations)
static int run(const Case& c, const char* what) {
    const int E = (int)c.size();
    size_t tot = 0;
    for (const Ev& v : c) tot += (size_t)v.n();
    double *ra = heap<double>(tot), *ri = heap<double>(tot), *mean = heap<double>(tot), *stdv = heap<double>(tot);
    ps::VitGatherEvent* ev = heap<ps::VitGatherEvent>((size_t)E);
    size_t off = 0;
    for (int e = 0; e < E; e++) {
        const Ev& v = c[e];
        ev[e] = {v.n(), (int64_t)off, v.has_index, v.refstart, v.refend};
        for (int t = 0; t < v.n(); t++) { ra[off + t] = v.ra[t]; ri[off + t] = v.ri[t]; mean[off + t] = v.mean[t]; stdv[off + t] = v.stdv[t]; }
        off += (size_t)v.n();
    }
    ps::VitGather g;
    ps::vit_gather({E, ev, ra, ri, mean, stdv}, &g);
    const Want w = naive(c);
    EXPECT(g.T == w.T);
    EXPECT(g.obsin.size() == (size_t)w.T * E * 4 && g.obsin.size() == w.obsin.size());
    const bool same = g.obsin.size() == w.obsin.size() && (w.obsin.empty() || memcmp(g.obsin.data(), w.obsin.data(), w.obsin.size() * sizeof(double)) == 0);
    EXPECT(same);
    if (g.T != w.T || !same) printf("  in: %s (T %d, want %d)\n", what, g.T, w.T);
    free(ra); free(ri); free(mean); free(stdv); free(ev);
    return g.T;
}

static int present(const Case& c, int position_row, int e, const Want& w) { return w.obsin[((size_t)position_row * c.size() + e) * 4 + 3] != 0.0; }

int main() {
    // a read without an aligned level in front of a live one: the walk starts at -1 and goes on
    { Case c = {unaligned(7), col0(plain(1, 60))}; EXPECT(run(c, "unaligned first") > 50); }
    { Case c = {unaligned(7), plain(1, 60)}; EXPECT(run(c, "unaligned first, nothing on column 0") == 0); }
    // the same next to -1 markers behind an aligned level 0: std::find meets them at position -1, which is kept
    {
        Case c = {unaligned(3), markers_behind_level0(1, 60), col0(plain(1, 60))};
        c[1].ra[1] = c[1].ri[1] = -1.0;
        const Want w = naive(c);
        EXPECT(present(c, 0, 1, w) && !present(c, 0, 0, w));
        run(c, "-1 markers");
    }
    // whole ref_index values past the largest refend: more positions than the reads are aligned to
    {
        Case c = {overhang(1, 40, 9), plain(1, 40)};
        const int last = std::max(c[0].refend, c[1].refend), first = std::min(c[0].refstart, c[1].refstart);
        EXPECT(run(c, "overhang") > last - first + 1);
    }
    // a position one of six reads covers: skipped.  Column 30 is cut out of five reads, the sixth holds it
    {
        Case c;
        for (int k = 0; k < 6; k++) {
            Ev e;
            for (int col = 10; col <= 50; col++) if (k == 0 || col != 30) e.level(col, col);
            e.span();
            c.push_back(e);
        }
        EXPECT(run(c, "one of six") == 40);
    }
    // a gap no read spans: the walk stops in front of it
    { Case c = {plain(5, 30, 20), plain(200, 260)}; EXPECT(run(c, "gap") < 40); }
    // an event of 0 levels; E = 1; 0 levels alone
    { Case c = {Ev(), col0(plain(1, 80))}; EXPECT(run(c, "empty event first") > 60); }
    { Case c = {plain(3, 80), Ev(), Ev()}; run(c, "empty events last"); }
    { Case c = {plain(1, 120)}; EXPECT(run(c, "E = 1") > 90); }
    { Case c = {Ev()}; EXPECT(run(c, "E = 1, no levels") == 0); }
    { Case c = {unaligned(5)}; EXPECT(run(c, "E = 1, unaligned") == 0); }
    // has_index false over arrays that look aligned
    { Case c = {no_index_over_arrays(1, 90), col0(plain(1, 70))}; EXPECT(run(c, "no index first") > 50); }
    { Case c = {plain(20, 70), no_index_over_arrays(1, 90)}; run(c, "no index last"); }
    { Case c = {no_index_over_arrays(1, 90)}; EXPECT(run(c, "no index alone") == 0); }
    // fractional and NaN ref_index; values the table must ignore
    for (int k = 0; k < 20; k++) { Case c = {holes(1 + rnd(5), 150), holes(1 + rnd(30), 200), plain(1, 100)}; run(c, "holes"); }
    for (int k = 0; k < 20; k++) { Case c = {huge(1 + rnd(5), 90), plain(1 + rnd(9), 100)}; run(c, "huge"); }
    { Case c = {huge(2, 50)}; run(c, "huge alone"); }
    // random compositions
    for (int k = 0; k < 400; k++) {
        Case c;
        const int E = 1 + rnd(7);
        const bool from0 = rnd(2) == 0;   // every read with levels begins on column 0: a walk that starts at -1 goes on
        for (int e = 0; e < E; e++) {
            const int from = from0 || rnd(4) == 0 ? 1 : 1 + rnd(60), to = from + rnd(220);
            switch (rnd(9)) {
                case 0: c.push_back(unaligned(rnd(12))); break;
                case 1: c.push_back(markers_behind_level0(from, to)); break;
                case 2: c.push_back(overhang(from, to, 1 + rnd(30))); break;
                case 3: c.push_back(holes(from, to)); break;
                case 4: c.push_back(huge(from, to)); break;
                case 5: c.push_back(no_index_over_arrays(from, to)); break;
                case 6: c.push_back(Ev()); break;
                default: c.push_back(plain(from, to)); break;
            }
            if (from0 && c.back().has_index) c.back() = col0(c.back());
            if (c.back().n() >= 300) { printf("an event of %d levels\n", c.back().n()); return 2; }
        }
        run(c, "random");
    }
    printf("checks=%ld failures=%ld\n", checks, bad);
    return bad ? 1 : 0;
}
