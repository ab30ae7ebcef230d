// Host check of the deterministic Viterbi back-trace (poreseq_amd/csrc/ps_vitpath.h), meant to be built with
// -fsanitize=address,undefined: every table is a heap block of exactly its own size, so a walk that indexes a row with -1 reads
// before the block (region at row 0) or is caught by the expected path (region at t_off > 0, where -1 lands in a neighbour's rows).
//
// Tables: live; dead from row 0; dead from a middle row; dead last row only; T = 1 (live and dead: never refused); a -1 off the
// path (not an error); a dead stretch that a live row interrupts (the named row is the first of the last stretch); the same
// tables as the second and third region of a concatenated table.  Expected results come from a separate bounds-checked walk here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../poreseq_amd/csrc/ps_vitpath.h"

static const int NS = 1024;
static long bad = 0, checks = 0;
static unsigned long long rs = 88172645463325252ull;
static int rnd(int n) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (int)(rs % (unsigned long long)n); }

#define EXPECT(c)                                                        \
    do {                                                                 \
        checks++;                                                        \
        if (!(c)) { bad++; printf("FAIL line %d: %s\n", __LINE__, #c); } \
    } while (0)

struct Table {
    int T;
    std::vector<int16_t> bp;   // [T][NS]
    explicit Table(int T_) : T(T_), bp((size_t)T_ * NS) {
        for (auto& b : bp) b = (int16_t)rnd(NS);
    }
    void kill_row(int t) { for (int s = 0; s < NS; s++) bp[(size_t)t * NS + s] = -1; }
    int16_t& at(int t, int s) { return bp[(size_t)t * NS + s]; }
};

// the rule restated with every index checked: -1 and the path, or the row to name
static long expect_walk(const Table& tb, int start, std::vector<int>* path) {
    path->assign(tb.T, -7);
    int c = start;
    for (int i = tb.T - 1; i >= 0; i--) {
        if (c < 0 || c >= NS) { printf("expect_walk: state out of range\n"); exit(2); }
        (*path)[i] = c;
        if (i == 0) break;
        const int q = tb.bp[(size_t)i * NS + c];
        if (q < 0) {
            int j = i;
            while (j > 0) {
                bool dead = true;
                for (int s = 0; s < NS; s++) if (tb.bp[(size_t)(j - 1) * NS + s] >= 0) dead = false;
                if (!dead) break;
                j--;
            }
            return j;
        }
        c = q;
    }
    return -1;
}

// run one region alone (its own heap block, t_off 0) and check against want_dead (-1: a path)
static void run_alone(const Table& tb, int start, long want_dead, const char* what) {
    std::vector<int> want;
    const long exp_dead = expect_walk(tb, start, &want);
    EXPECT(exp_dead == want_dead);
    int16_t* blk = (int16_t*)malloc(tb.bp.size() * sizeof(int16_t) + (tb.bp.empty() ? 1 : 0));
    for (size_t k = 0; k < tb.bp.size(); k++) blk[k] = tb.bp[k];
    int* path = (int*)malloc(sizeof(int) * (size_t)tb.T);
    for (int i = 0; i < tb.T; i++) path[i] = -7;
    const int64_t got = ps::vit_follow_bp(blk, 0, tb.T, NS, start, path);
    EXPECT(got == want_dead);
    bool same = true;
    for (int i = 0; i < tb.T; i++) same = same && path[i] == want[i];   // (entries below a stop stay untouched in both)
    EXPECT(same);
    if (want_dead < 0) for (int i = 0; i < tb.T; i++) EXPECT(path[i] >= 0 && path[i] < NS);
    if (got != want_dead || !same) printf("  in: %s\n", what);
    free(path);
    free(blk);
}

int main() {
    const int Ts[] = {2, 3, 9, 17, 40};
    // live tables
    for (int T : Ts) { Table tb(T); run_alone(tb, rnd(NS), -1, "live"); }
    // T = 1: live and dead, never refused (bp[0][.] is not followed)
    { Table tb(1); run_alone(tb, 5, -1, "T = 1 live"); }
    { Table tb(1); tb.kill_row(0); run_alone(tb, 0, -1, "T = 1 dead"); }
    for (int T : Ts) {
        // dead from row 0
        { Table tb(T); for (int t = 0; t < T; t++) tb.kill_row(t); run_alone(tb, 0, 0, "dead from row 0"); }
        // dead from a middle row
        if (T >= 3) { Table tb(T); const int m = T / 2; for (int t = m; t < T; t++) tb.kill_row(t); run_alone(tb, rnd(NS), m, "dead from a middle row"); }
        // dead last row only
        { Table tb(T); tb.kill_row(T - 1); run_alone(tb, rnd(NS), T - 1, "dead last row"); }
        // a dead stretch, a live row, a dead stretch to the end: the last stretch's first row is named
        if (T >= 9) { Table tb(T); tb.kill_row(1); tb.kill_row(2); for (int t = 4; t < T; t++) tb.kill_row(t); run_alone(tb, 3, 4, "two dead stretches"); }
        // row 0 dead alone under a live table: bp[0] is not followed
        { Table tb(T); tb.kill_row(0); run_alone(tb, rnd(NS), -1, "row 0 dead, rest live"); }
    }
    // a -1 off the path is no error; the same -1 on the path is, and names its own row (the row before it is live)
    {
        Table tb(9);
        std::vector<int> p;
        const int start = 77;
        expect_walk(tb, start, &p);
        for (int t = 1; t < 9; t++) tb.at(t, (p[t] + 1) % NS) = -1;
        tb.at(0, p[0]) = -1;
        run_alone(tb, start, -1, "-1 off the path");
        tb.at(5, p[5]) = -1;
        run_alone(tb, start, 5, "-1 on the path, partly dead row");
        // half of every row dead (a partly dead row of the recursion), path on the live half
        Table hb(9);
        for (int t = 0; t < 9; t++) for (int s = 0; s < NS; s++) hb.at(t, s) = (s & 1) ? (int16_t)(2 * rnd(NS / 2) + 1) : (int16_t)-1;
        run_alone(hb, 1, -1, "odd states live");
        run_alone(hb, 2, 8, "even start dead");
    }
    // regions at t_off > 0 of a concatenated table: (live 9, dead-from-middle 17, T = 0, live 5, dead-from-row-0 3, T = 1 dead)
    {
        std::vector<Table> regs;
        regs.emplace_back(9);
        regs.emplace_back(17); for (int t = 8; t < 17; t++) regs.back().kill_row(t);
        regs.emplace_back(0);
        regs.emplace_back(5);
        regs.emplace_back(3); for (int t = 0; t < 3; t++) regs.back().kill_row(t);
        regs.emplace_back(1); regs.back().kill_row(0);
        const long want_dead[] = {-1, 8, -1, -1, 0, -1};
        size_t rows = 0;
        for (auto& r : regs) rows += r.T;
        int16_t* all = (int16_t*)malloc(rows * NS * sizeof(int16_t));
        size_t off = 0;
        for (auto& r : regs) { for (size_t k = 0; k < r.bp.size(); k++) all[off * NS + k] = r.bp[k]; off += r.T; }
        off = 0;
        for (size_t r = 0; r < regs.size(); r++) {
            const int T = regs[r].T, start = T ? rnd(NS) : 0;
            std::vector<int> want;
            const long exp_dead = T ? expect_walk(regs[r], start, &want) : -1;
            EXPECT(exp_dead == want_dead[r]);
            int* path = (int*)malloc(sizeof(int) * (size_t)(T ? T : 1));
            for (int i = 0; i < T; i++) path[i] = -7;
            const int64_t got = ps::vit_follow_bp(all, (int64_t)off, T, NS, start, path);
            EXPECT(got == want_dead[r]);
            for (int i = 0; i < T; i++) EXPECT(path[i] == want[i]);
            free(path);
            off += T;
        }
        free(all);
    }
    printf("checks=%ld failures=%ld\n", checks, bad);
    return bad ? 1 : 0;
}
