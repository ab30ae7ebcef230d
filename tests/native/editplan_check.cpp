// Host check of the edit plan's arithmetic (poreseq_amd/csrc/ps_editplan.h) against brute force: every edit is applied to the whole
// sequence (apply_edit, ps_greedy.h) and the states of the whole edited sequence are the yardstick of edited_window's 12-base
// look-back; sizes, kept columns, old-score columns and size classes are held to their formulae restated naively; point_layout to
// FindPointMutations' list itself.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "../../poreseq_amd/csrc/ps_editplan.h"

using namespace ps;

static long bad = 0;
#define CHECK(cond) do { if (!(cond)) { if (bad++ < 10) printf("line %d: %s (case %ld)\n", __LINE__, #cond, trial); } } while (0)

static unsigned long long rnd_state = 88172645463325252ull;
static unsigned long long rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }
static int below(int n) { return (int)(rnd() % (unsigned long long)n); }

// ACGT with an occasional N, '-' or a byte >= 0x80 (`odd` in 1000)
static std::string rand_seq(int len, int odd) {
    static const char other[] = {'N', '-', (char)0x80, (char)0xF3};
    std::string s(len, 'A');
    for (char& c : s) c = below(1000) < odd ? other[below(4)] : "ACGT"[below(4)];
    return s;
}

static Mut rand_edit(const std::string& b) {
    const int L = (int)b.size();
    const int where[] = {0, 1, L - 1, L, L + 1};
    Mut m;
    m.start = below(3) ? below(L + 2) : where[below(5)];
    const int kind = below(3);   // substitution, insertion, deletion
    const int olen = kind == 1 ? 0 : below(41), mlen = kind == 2 ? 0 : below(41);
    // orig as the sequence has it where it can (its content is never read, only its length), running past the end now and then
    for (int i = 0; i < olen; i++) m.orig.push_back(m.start + i < L ? b[m.start + i] : 'A');
    m.mut = rand_seq(mlen, 30);
    return m;
}

static int clampc(int c, int C) { return (c < 0 || c > C) ? C : c; }
static int naive_class(int ncol) { if (ncol <= 7) return 4; if (ncol <= 8) return 0; if (ncol <= 16) return 1; if (ncol <= 32) return 2; return 3; }

// one list on one sequence at one scoring width: every table of its plan
static void check_list(const std::string& b, int WS, const std::vector<Mut>& muts, int nth, long trial) {
    const int L = (int)b.size(), C = (int)states_of(b).size(), M = (int)muts.size();
    CHECK(C == (L >= 5 ? L - 4 : 0));
    EditPlan p;
    plan_edits(b, C, WS, muts, &p);
    CHECK(!p.bad_start && p.M == M);
    plan_keep(C, &p);
    plan_tables(b, muts, &p, nth);
    int ncolmax = 1, extra = 0;
    std::set<int> want[2], r0_seen;
    std::vector<int> want_cls[SCORE_CLASSES];
    CHECK((int)p.states.size() == M * p.ncolmax);
    for (int i = 0; i < M; i++) {
        const Mut& m = muts[i];
        const std::vector<int> full = states_of(apply_edit(b, m));   // Sequence(original, mut).states
        const int Cm = (int)full.size();
        const int skip = m.start > L ? 1 : 0;
        const int sidx = m.start - 4 > 0 ? m.start - 4 : 0;
        int ncol = std::min((int)m.mut.size() + 6, std::max(0, Cm - sidx));
        if (WS == 0 || skip) ncol = 0;
        CHECK(p.start[i] == m.start && p.mlen[i] == (int)m.mut.size() && p.cm[i] == Cm && p.skip[i] == skip && p.ncol[i] == ncol);
        ncolmax = std::max(ncolmax, ncol);
        if (!skip) extra = std::max(extra, sidx + ncol + 1 - (C + 1));
        // the new columns' states: the slice of the whole edited sequence's, -1 beyond its end and beyond ncol
        for (int c = 0; c < p.ncolmax; c++) {
            const int got = p.states[(size_t)i * p.ncolmax + c];
            CHECK(got == (c < ncol && sidx + c < Cm ? full[sidx + c] : -1));
        }
        want_cls[naive_class(ncol)].push_back(i);
        if (skip) { CHECK(p.oldidx[i] == 0); continue; }
        const int r0 = m.start - 3 > 1 ? m.start - 3 : 1;
        CHECK(p.oldidx[i] >= 0 && p.oldidx[i] < (int)p.r0s.size() && p.r0s[p.oldidx[i]] == r0);
        const int tcol = std::min(m.start + (int)m.mut.size() + 1, sidx + ncol);
        const int fwd[2] = {clampc(sidx, C), clampc(r0, C)}, bwd[2] = {clampc(Cm - tcol + 1, C), clampc(C - r0 + 1, C)};
        for (int q = 0; q < 2; q++) { if (fwd[q] > 0) want[0].insert(fwd[q]); if (bwd[q] > 0) want[1].insert(bwd[q]); }
    }
    CHECK(p.ncolmax == ncolmax && p.extra == std::max(extra, 0) + 2);
    for (int d = 0; d < 2; d++) {   // the kept columns are exactly the wanted set, numbered densely in ascending order
        CHECK((int)p.keep[d].size() == C + 2 && p.nkeep[d] == (int)want[d].size());
        int next = 0;
        for (int c = 0; c < (int)p.keep[d].size(); c++) {
            if (want[d].count(c)) { CHECK(p.keep[d][c] == next); next++; }
            else CHECK(p.keep[d][c] == -1);
        }
    }
    CHECK(p.nr0 == (int)p.r0s.size());
    for (int r : p.r0s) { CHECK(!r0_seen.count(r)); r0_seen.insert(r); }
    for (int k = 0; k < SCORE_CLASSES; k++) CHECK(p.cls[k] == want_cls[k]);   // a partition of 0 .. M - 1, ascending in each class
}

static void check_points(const std::string& b, long trial) {
    const size_t n = states_of(b).size();
    std::vector<Mut> list;
    std::vector<int> first, triv;
    point_edits(b, n, &list);
    point_layout(b, n, &first, &triv);
    CHECK(first.size() == n + 1 && triv.size() == n && first[n] == (int)list.size());
    for (size_t p = 0; p < n && first[n] == (int)list.size(); p++) {
        int at = first[p];
        const char* own = strchr("ACGT", b[p]);
        CHECK(triv[p] == (own && b[p] ? (int)(own - "ACGT") + 1 : 0));
        CHECK(list[at].start == (int)p && list[at].orig == std::string(1, b[p]) && list[at].mut.empty());   // the deletion
        at++;
        for (int k = 0; k < 4; k++) {   // substitutions in ACGT order, the base's own left out
            if (triv[p] == k + 1) continue;
            CHECK(list[at].start == (int)p && list[at].orig == std::string(1, b[p]) && list[at].mut == std::string(1, "ACGT"[k]));
            at++;
        }
        for (int k = 0; k < 4; k++, at++) CHECK(list[at].start == (int)p && list[at].orig.empty() && list[at].mut == std::string(1, "ACGT"[k]));
        CHECK(at == first[p + 1]);
    }
}

int main(int argc, char** argv) {
    const long trials = argc > 1 ? atol(argv[1]) : 4000;
    long trial = -1;
    // the size classes and the lanes k_score is launched with for them: the smallest group that holds the columns; 64 is chunked
    for (int ncol = 0; ncol <= 100; ncol++) {
        const int k = score_class(ncol), lanes = score_class_lanes(k);
        CHECK(k == naive_class(ncol) && k >= 0 && k < SCORE_CLASSES);
        CHECK(lanes == (ncol <= 7 ? 7 : ncol <= 8 ? 8 : ncol <= 16 ? 16 : ncol <= 32 ? 32 : 64));
    }
    const int widths[3] = {0, 1, 8};
    for (trial = 0; trial < trials; trial++) {
        const std::string b = rand_seq(5 + below(76), trial % 3 ? 40 : 0);
        std::vector<Mut> muts(1 + below(12));
        for (Mut& m : muts) m = rand_edit(b);
        check_list(b, widths[trial % 3], muts, 1, trial);
        check_points(b, trial);
    }
    {   // a negative start is refused before anything is sized
        std::vector<Mut> muts(2);
        muts[1].start = -1;
        EditPlan p;
        plan_edits("ACGTACGT", 4, 8, muts, &p);
        CHECK(p.bad_start);
    }
    {   // from 4096 edits on plan_tables fills the states on several threads: the same tables as on one
        const std::string b = rand_seq(80, 40);
        std::vector<Mut> muts(5000);
        for (Mut& m : muts) m = rand_edit(b);
        EditPlan p1, p8;
        plan_edits(b, 76, 8, muts, &p1); plan_keep(76, &p1); plan_tables(b, muts, &p1, 1);
        plan_edits(b, 76, 8, muts, &p8); plan_keep(76, &p8); plan_tables(b, muts, &p8, 8);
        CHECK(p1.states == p8.states && p1.r0s == p8.r0s && p1.oldidx == p8.oldidx && p1.keep[0] == p8.keep[0] && p1.keep[1] == p8.keep[1]);
        for (int k = 0; k < SCORE_CLASSES; k++) CHECK(p1.cls[k] == p8.cls[k]);
        check_list(b, 8, muts, 8, trial);
    }
    printf("trials=%ld failures=%ld\n", trials, bad);
    return bad ? 1 : 0;
}
