// sw_layout_check.cpp — host check of the Smith-Waterman checkpoint layout (poreseq_amd/csrc/ps_swplan.h): that the fills, the
// traceback and the allocation agree on where every rowsave / colsave / blkmax entry lives.
//
// Batches of several pairs are laid out by sw_lay_out as sw_launch does, each pool a heap block of exactly its total size (the program
// runs under AddressSanitizer).  For every pair the program walks the stores of the fill that serves it (k_sw_fill<K, WW> /
// k_sw_fill_pk<WW, false> on the full matrix, k_sw_fill_pk<SWBW, true> in band mode) under the kernels' guards and with the
// compile-time address forms they use, tagging each int with (pair, kind, block, column / row); then the loads of k_sw_trace with the
// run-time forms: the linear scan of the block maxima, the start-cell search (sw_tile<K, 1> of every block whose maximum the fill
// stored: the others hold the launch's zero and never equal a positive best) and sw_tile<1, 2> of every 64 x 64 tile of the matrix or
// band region, plus the boundary-column loads of the fills themselves.  It asserts that every index lies inside its own pair's part of
// the pool, that no two entries share an int, and that every rowsave / colsave entry loaded carries the tag of the very entry the
// load means — those pools are never cleared, so this is the check that no uninitialised checkpoint is read (blkmax is cleared by
// sw_launch: any index inside the pair's part will do).  Last, sw_pair_bytes against fixed values: the chunk boundaries must not move.
// Prints "failures=N".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../poreseq_amd/csrc/ps_swplan.h"

using namespace ps;

static long g_fail = 0, g_stores = 0, g_loads = 0;

struct Pool {
    int64_t* tag; int64_t n;          // one tag per int of the pool, 0: never stored
    explicit Pool(int64_t n_) : tag(new int64_t[n_]()), n(n_) {}
    ~Pool() { delete[] tag; }
};
struct Part { int64_t lo, hi; };      // a pair's part of a pool
struct PairCtx {
    SwPair p; int id, K, WW;
    Part row, col, blk;
};

static int64_t key(int id, int a, int b) { return ((int64_t)(id + 1) << 44) | ((int64_t)a << 22) | (int64_t)b; }

static void report(const PairCtx& c, const char* what, const char* pool, int64_t idx, int a, int b) {
    if (g_fail++ < 10)
        printf("%s: %s[%lld] (%d, %d) of pair %d: n1 %d n2 %d wb %d K %d WW %d\n", what, pool, (long long)idx, a, b, c.id, c.p.n1, c.p.n2, c.p.wb, c.K, c.WW);
}

static void store(Pool& P, const Part& part, const char* pool, const PairCtx& c, int64_t idx, int a, int b) {
    g_stores++;
    if (idx < part.lo || idx >= part.hi) return report(c, "store outside the pair's part", pool, idx, a, b);
    if (P.tag[idx]) return report(c, "two entries share an int", pool, idx, a, b);
    P.tag[idx] = key(c.id, a, b);
}
static void load(const Pool& P, const Part& part, const char* pool, const PairCtx& c, int64_t idx, int a, int b) {
    g_loads++;
    if (idx < part.lo || idx >= part.hi) return report(c, "load outside the pair's part", pool, idx, a, b);
    if (P.tag[idx] != key(c.id, a, b)) report(c, P.tag[idx] ? "load of another entry" : "load of an entry the fill never stored", pool, idx, a, b);
}

// ---- the stores (and boundary-column loads) of one pair's fill: k_sw_fill / k_sw_fill_pk, guard for guard ------------------------
template <bool BAND>
static void fill(const PairCtx& c, Pool& row, Pool& col, Pool& blk) {
    const SwPair& p = c.p;
    const int K = BAND ? PKK : c.K, WP = BAND ? 1 : c.WW;   // band: one wave per strip, the strips one after the other
    for (int ss = 0; ss * WP * 64 * K < p.n2; ss++)
        for (int w = 0; w < WP; w++) {
            const int gw = BAND ? ss : ss * c.WW + w, wfirst = gw * 64 * K;
            if (wfirst >= p.n2) continue;   // wave_on
            const SwWin win = band_win<BAND>(p, ss), pwin = band_left<BAND>(win);
            const int r0 = 64 * band_q0<BAND>(win), rend = col_hi<BAND>(p, win), pend = col_hi<BAND>(p, pwin);
            const int cb = r0 / SWB, ce = (rend + SWB - 1) / SWB;
            if (w == 0 && gw > 0) {         // the left neighbour's boundary column H(*, wfirst), read by the strip's first wave
                const int64_t cprev = col_base<BAND>((int64_t)0, p, wfirst >> 6, pwin);
                if (BAND && r0 > 0 && r0 <= pend) load(col, c.col, "colsave", c, cprev + r0, wfirst >> 6, r0);
                for (int ch = cb; ch < ce; ch++)
                    for (int l = 0; l < SWB; l++)
                        if (ch * SWB + l < rend && ch * SWB + 1 + l <= pend) load(col, c.col, "colsave", c, cprev + ch * SWB + 1 + l, wfirst >> 6, ch * SWB + 1 + l);
            }
            for (int l = 0; l < 64; l++) {
                const int jbase = wfirst + l * K;
                const bool keeps = ((jbase + K) & 63) == 0 && jbase + K <= p.n2;
                const int cc = (jbase + K) >> 6;
                const int64_t csave = col_base<BAND>((int64_t)0, p, cc, win);
                if (keeps) store(col, c.col, "colsave", c, csave + r0, cc, r0);
                for (int ch = cb; ch < ce; ch++) {
                    const int i0 = ch * SWB;
                    if (keeps)
                        for (int r = 0; r < SWB; r++) if (i0 + r < rend) store(col, c.col, "colsave", c, csave + i0 + r + 1, cc, i0 + r + 1);
                    const int iend = std::min(i0 + SWB, rend);
                    if ((iend & 63) == 0 || iend == rend) {   // row block q complete
                        const int q = (iend - 1) >> 6;
                        if (l == 0) store(blk, c.blk, "blkmax", c, bm_index<BAND>(p, q, gw, win), q, gw);
                        if (iend < rend) {
                            const int64_t rs = rs_index<BAND>(p, q + 1, jbase, ss);
                            for (int k = 0; k < K; k++) if (jbase + k < p.n2) store(row, c.row, "rowsave", c, rs + k, q + 1, jbase + k);
                        }
                    }
                }
            }
        }
}

// ---- the loads of sw_tile<K, MODE>: rows 64q + 1 .. 64q + nrows of the strip of 64 K columns at c0 ---------------------------------
static void tile(const PairCtx& c, const Pool& row, const Pool& col, int K, int q, int c0, int nrows) {
    const SwPair& p = c.p;
    const bool top = q > band_q0(p, c0 / SWBS);
    for (int l = 0; l < 64; l++) {
        const int jbase = c0 + l * K;
        const int64_t rs = rs_index(p, q, jbase);
        for (int k = 0; k < K; k++) if (jbase + k < p.n2 && top) load(row, c.row, "rowsave", c, rs + k, q, jbase + k);
    }
    if (c0 > 0) {
        const int64_t cprev = col_base(p, c0 >> 6);
        const int chi = col_hi(p, c0 >> 6);
        if (64 * q <= chi) load(col, c.col, "colsave", c, cprev + 64 * q, c0 >> 6, 64 * q);
        for (int l = 0; l < nrows; l++) if (64 * q + 1 + l <= chi) load(col, c.col, "colsave", c, cprev + 64 * q + 1 + l, c0 >> 6, 64 * q + 1 + l);
    }
}

// ---- the loads of k_sw_trace<K, *> ---------------------------------------------------------------------------------------------
static void trace(const PairCtx& c, const Pool& row, const Pool& col, const Pool& blk) {
    const SwPair& p = c.p;
    const int K = p.wb ? PKK : c.K;
    for (int k = 0; k < bm_count(p); k++) {   // the linear scan for the maximum
        g_loads++;
        if (bm_base(p) + k < c.blk.lo || bm_base(p) + k >= c.blk.hi) report(c, "scan outside the pair's part", "blkmax", bm_base(p) + k, k, 0);
    }
    for (int gw = 0; gw < p.ngw; gw++)        // the start cell: the blocks whose maximum is the best
        for (int q = band_q0(p, gw); q < band_q1(p, gw); q++) {
            const int64_t b = bm_index(p, q, gw);
            g_loads++;
            if (b < c.blk.lo || b >= c.blk.hi) { report(c, "load outside the pair's part", "blkmax", b, q, gw); continue; }
            if (!blk.tag[b]) continue;        // (cleared by the launch: never the positive best)
            if (blk.tag[b] != key(c.id, q, gw)) report(c, "load of another entry", "blkmax", b, q, gw);
            tile(c, row, col, K, q, gw * 64 * K, std::min(64, p.n1 - 64 * q));
        }
    for (int cb = 0; 64 * cb < p.n2; cb++) {  // the walk: any tile of the matrix or band region, entered at its last row
        const int s = 64 * cb / SWBS;
        for (int q = band_q0(p, s); q < band_q1(p, s); q++) tile(c, row, col, 1, q, 64 * cb, std::min(64, p.n1 - 64 * q));
    }
}

// ---- batches ----------------------------------------------------------------------------------------------------------------------
struct Case { int n1, n2, wb; };

static void run_batch(const std::vector<Case>& cases, int K, int WW, SwForm form, int id0) {
    const int np = (int)cases.size();
    std::vector<PairCtx> ctx(np);
    std::vector<int> wb(np);
    SwPools tot;
    for (int k = 0; k < np; k++) {     // input order, as sw_launch lays out
        PairCtx& c = ctx[k];
        const SwPools before = tot;
        sw_lay_out(c.p, cases[k].n1, cases[k].n2, cases[k].wb, form, K, WW, tot);
        c.id = id0 + k; c.K = K; c.WW = WW; wb[k] = cases[k].wb;
        c.row = {before.row, tot.row}; c.col = {before.col, tot.col}; c.blk = {before.blk, tot.blk};
        if (c.p.row_off != before.row || c.p.col_off != before.col || c.p.blk_off != before.blk || c.p.out_off != before.out || c.p.res_off != before.res ||
            tot.res - before.res != SW_RES || tot.out - before.out != (form == SW_LISTS ? 2 * ((int64_t)c.p.n1 + c.p.n2 + 2) : (form == SW_MAP ? c.p.n1 + 2 : 0)))
            report(c, "offsets do not follow the totals", "pools", 0, 0, 0);
    }
    Pool row(tot.row), col(tot.col), blk(tot.blk);
    const std::vector<int> order = sw_device_order(wb);   // both launches' fills run before either traceback reads
    for (int k : order) { if (ctx[k].p.wb) fill<true>(ctx[k], row, col, blk); else fill<false>(ctx[k], row, col, blk); }
    for (int k : order) trace(ctx[k], row, col, blk);
}

int main() {
    const int LEN[] = {1, 2, 63, 64, 65, 127, 128, 511, 512, 513, 1023, 1025, 2047, 2048, 2049, 4097};
    const int WB[] = {0, 64, 128, 1024};
    const int KWW[5][2] = {{4, 8}, {8, 8}, {16, 8}, {8, 16}, {16, 16}};   // (the last two: one workgroup per pair; every n2 here fits 16 x 64 x K)
    // every (n1, n2) of LEN on the full matrix in every fill form; every (n1, n2, band width) once, spread over the forms' batches
    std::vector<Case> stream[5];
    int nband = 0;
    for (int n1 : LEN)
        for (int n2 : LEN) {
            for (int t = 0; t < 5; t++) stream[t].push_back({n1, n2, 0});
            for (int w = 1; w < 4; w++) stream[nband++ % 5].push_back({n1, n2, WB[w]});
        }
    std::mt19937 g(20240611);
    for (int t = 0; t < 300; t++) stream[g() % 5].push_back({1 + (int)(g() % 5000), 1 + (int)(g() % 5000), WB[g() % 4]});
    int id = 0, nbatch = 0;
    for (int t = 0; t < 5; t++) {
        std::shuffle(stream[t].begin(), stream[t].end(), g);   // batches mix lengths and modes
        for (size_t k0 = 0; k0 < stream[t].size(); k0 += 7) {
            const std::vector<Case> b(stream[t].begin() + k0, stream[t].begin() + std::min(stream[t].size(), k0 + 7));
            run_batch(b, KWW[t][0], KWW[t][1], (SwForm)(nbatch++ % 3), id);
            id += (int)b.size();
        }
    }
    // sw_pair_bytes, as the parent commit returned it: these values cut the chunks
    const struct { int n1, n2, wb; SwForm form; double bytes; } PIN[] = {
        {1, 1, 0, SW_LISTS, 76.6875},
        {513, 511, 0, SW_LISTS, 45396.3125},
        {10000, 10007, 0, SW_LISTS, 12754511.4375},
        {10000, 10007, 0, SW_SUMMARY, 12594439.4375},
        {12084, 11890, 0, SW_MAP, 18062562.125},
        {3000, 2987, 128, SW_LISTS, 342294.6875},
        {10000, 10007, 1024, SW_LISTS, 3413661.4375},
        {10000, 10007, 1024, SW_SUMMARY, 3253589.4375},
        {4097, 4097, 64, SW_MAP, 351380.0625},
        {700, 13000, 1024, SW_SUMMARY, 4225136.5},
    };
    for (const auto& x : PIN)
        if (sw_pair_bytes(x.n1, x.n2, x.wb, x.form) != x.bytes) {
            if (g_fail++ < 10) printf("sw_pair_bytes(%d, %d, %d, %d) = %.17g, expected %.17g\n", x.n1, x.n2, x.wb, (int)x.form, sw_pair_bytes(x.n1, x.n2, x.wb, x.form), x.bytes);
        }
    printf("pairs=%d batches=%d stores=%ld loads=%ld failures=%ld\n", id, nbatch, g_stores, g_loads, g_fail);
    return g_fail ? 1 : 0;
}
