// Host check of the output plan of the own-sequence statistics calls (poreseq_amd/csrc/ps_ownplan.h), meant to be built with
// -fsanitize=address,undefined.  Seeded random calls of every kind — 0 to 6 regions of 0 to 7 events of 0 to 700 levels, regions
// without events and events without levels among them, random wants per region, 1 to 256 groups — with and without a realignment
// where the kind allows it (MoveStats always has one, Posterior and its scratch never).
//
// Every segment of the plan lies inside the bytes to ensure, every copied one inside the bytes that come back, no two overlap, each
// starts on a multiple of its element size, the scratch lies behind everything copied, every job's levels lie inside their segment
// behind those of the job before — and totals and every offset equal a naive restatement written out below in the terms the three
// hand-written layouts used before there was a plan (stats_tail: records or tables, then the scores; moves_place: records, scores,
// columns, step codes; posterior(): records, emit, col, then the per-row sums that do not come back), so it also documents that the
// layout did not move.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../poreseq_amd/csrc/ps_ownplan.h"

using namespace ps;
static long bad = 0, checks = 0;
static unsigned long long rs = 88172645463325252ull;
static int rnd(int n) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (int)(rs % (unsigned long long)n); }

#define EXPECT(c)                                                        \
    do {                                                                 \
        checks++;                                                        \
        if (!(c)) { bad++; printf("FAIL line %d: %s\n", __LINE__, #c); } \
    } while (0)

// the layout as the three tails stated it: offsets and sizes in bytes, SIZE_MAX for an output the kind does not have
struct Naive {
    size_t main_bytes = 0, sc_off = SIZE_MAX, col_off = SIZE_MAX, step_off = SIZE_MAX, emit_off = SIZE_MAX, pcol_off = SIZE_MAX, row_off = SIZE_MAX;
    size_t out_bytes = 0, ensure_bytes = 0;
    double alg = 0;
    std::vector<size_t> lev_off;
    std::vector<int> job0, tab0;
    int maxE = 0, maxG = 0;
};
static Naive restate(const OwnView& v) {
    Naive x;
    const size_t nj = v.jobs.size();
    bool per_level = false;
    size_t levels = 0, rows = 0, q = 0;
    double cells = 0;
    for (const OwnView::Job& j : v.jobs) { x.lev_off.push_back(levels); levels += (size_t)j.n0; cells += (double)j.C * (2.0 * j.W + 1 < j.n0 ? 2.0 * j.W + 1 : j.n0); }
    for (const OwnView::Region& r : v.regs) {
        per_level |= r.levels;
        x.job0.push_back((int)q); q += (size_t)r.E;
        x.tab0.push_back((int)rows);
        if (v.kind == OwnKind::KmerStats) { rows += (size_t)r.ngroups; if (r.ngroups > x.maxG) x.maxG = r.ngroups; }
        if (r.E > x.maxE) x.maxE = r.E;
    }
    switch (v.kind) {
    case OwnKind::Score: break;
    case OwnKind::AlignStats: case OwnKind::KmerStats: {   // stats_tail
        const bool kmer = v.kind == OwnKind::KmerStats;
        x.main_bytes = kmer ? rows * 1024 * sizeof(ps_kmer_cell) : nj * sizeof(ps_event_stats);
        x.alg = (kmer ? 24.0 : 16.0) * (double)levels + (double)x.main_bytes;
        x.out_bytes = x.main_bytes + (v.re ? nj * sizeof(double) : 0);
        if (v.re) x.sc_off = x.main_bytes;
        x.ensure_bytes = x.out_bytes;
        break;
    }
    case OwnKind::MoveStats:                               // moves_place
        x.main_bytes = x.sc_off = nj * sizeof(ps_event_moves);
        x.col_off = x.sc_off + nj * sizeof(double);
        x.step_off = x.col_off + (per_level ? levels * sizeof(int32_t) : 0);
        x.out_bytes = x.ensure_bytes = x.step_off + (per_level ? levels : 0);
        x.alg = (per_level ? 13.0 : 8.0) * (double)levels + (double)x.sc_off;
        if (!per_level) x.col_off = x.step_off = SIZE_MAX;
        break;
    case OwnKind::Posterior:                               // posterior()
        x.main_bytes = x.emit_off = nj * sizeof(ps_event_posterior);
        x.pcol_off = x.emit_off + (per_level ? levels * sizeof(double) : 0);
        x.out_bytes = x.row_off = x.pcol_off + (per_level ? levels * sizeof(double) : 0);
        x.ensure_bytes = x.out_bytes + levels * 8 * sizeof(double);
        x.alg = cells;
        if (!per_level) x.emit_off = x.pcol_off = SIZE_MAX;
        if (!levels) x.row_off = SIZE_MAX;
        break;
    }
    return x;
}

static void check(const OwnView& v) {
    const OwnPlan p = lay_out(v);
    const Naive x = restate(v);
    const size_t want_at[OO_COUNT] = {0, x.sc_off, x.col_off, x.step_off, x.emit_off, x.pcol_off, x.row_off};
    EXPECT(p.nj == v.jobs.size() && p.back_bytes == x.out_bytes && p.ensure_bytes == x.ensure_bytes && p.bytes[OO_MAIN] == x.main_bytes);
    EXPECT(p.alg_bytes == x.alg && p.maxE == x.maxE && p.maxG == x.maxG);
    EXPECT(p.lev_off == x.lev_off && p.job0 == x.job0 && p.tab0 == x.tab0);
    for (int o = 0; o < OO_COUNT; o++) {
        const size_t el = own_out_elem(v.kind, (OwnOut)o);
        EXPECT(p.bytes[o] == own_out_bytes(v, p, (OwnOut)o));
        if (!p.bytes[o]) { EXPECT(o == OO_MAIN || want_at[o] == SIZE_MAX || p.nj == 0 || (o >= OO_COL && p.levels == 0)); continue; }
        EXPECT(p.at[o] == want_at[o]);
        EXPECT(el > 0 && p.at[o] % el == 0 && p.bytes[o] % el == 0);
        EXPECT(p.at[o] + p.bytes[o] <= p.ensure_bytes);
        if (o != OO_ROW) EXPECT(p.at[o] + p.bytes[o] <= p.back_bytes);
        else EXPECT(p.at[o] >= p.back_bytes);
        for (int u = 0; u < o; u++) EXPECT(!p.bytes[u] || p.at[u] + p.bytes[u] <= p.at[o]);
        if (o < OO_COL) continue;
        // the per-level outputs through the accessor the descriptors and the scatter use, on a heap block of the buffer's size
        std::vector<char> buf(p.ensure_bytes);
        const size_t per = o == OO_ROW ? 8 : 1;
        size_t end = p.at[o];
        for (size_t q = 0; q < p.nj; q++) {
            const char* lo = p.level<char>(buf.data(), (OwnOut)o, q, per * el);
            EXPECT(lo == buf.data() + end);
            end += (size_t)v.jobs[q].n0 * per * el;
        }
        EXPECT(end == p.at[o] + p.bytes[o]);
    }
    if (v.kind != OwnKind::Score && p.nj) {
        std::vector<char> buf(p.ensure_bytes);
        const size_t el = own_out_elem(v.kind, OO_MAIN);
        const size_t n_main = v.kind == OwnKind::KmerStats ? p.rows * PS_N_STATES : p.nj;
        EXPECT(p.item<char>(buf.data(), OO_MAIN, n_main * el) == buf.data() + p.bytes[OO_MAIN]);
    }
}

int main() {
    const OwnKind kinds[] = {OwnKind::Score, OwnKind::AlignStats, OwnKind::KmerStats, OwnKind::MoveStats, OwnKind::Posterior};
    long cases = 0;
    for (int it = 0; it < 800; it++)
        for (OwnKind kind : kinds)
            for (int re = 0; re < 2; re++) {
                if ((kind == OwnKind::MoveStats || kind == OwnKind::Score) && !re) continue;
                if (kind == OwnKind::Posterior && re) continue;
                OwnView v;
                v.kind = kind; v.re = re != 0;
                const int R = rnd(7);
                for (int k = 0; k < R; k++) {
                    OwnView::Region r;
                    r.E = rnd(3) ? rnd(8) : 0;
                    r.ngroups = kind == OwnKind::KmerStats ? 1 + rnd(256) : 0;
                    r.levels = (kind == OwnKind::MoveStats || kind == OwnKind::Posterior) && rnd(2);
                    v.regs.push_back(r);
                    const int C = 1 + rnd(400), W = rnd(320);
                    for (int e = 0; e < r.E; e++) v.jobs.push_back({rnd(4) ? rnd(701) : 0, C, W});
                }
                check(v);
                cases++;
            }
    printf("cases=%ld checks=%ld failures=%ld\n", cases, checks, bad);
    return bad ? 1 : 0;
}
