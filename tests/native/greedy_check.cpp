// Host check of the library's greedy pass of MakeMutations (poreseq_amd/csrc/ps_greedy.h: index sort with three branches, flat
// arrays) on an AlignData WITHOUT events, where re-scoring gives -1e-6 everywhere and MakeMutations is pure list logic:
//   1. against a checker library (the oracle or the reference build) through the C ABI of include/poreseq_hip.h: mutated-base count
//      and final sequence of ps_make_mutations;
//   2. against the plain statement of the reference's rule below (std::sort on the records themselves), which also yields what the
//      C ABI does not show: the deferred list handed to the re-scoring, entry by entry, with its starts.
// Random lists over random sequences of 5 to 400 bases: sizes 0 .. 700 (16 / 17 straddle libstdc++'s insertion-sort threshold) and, one
// list in 41, 701 .. 3 000, under each of four score profiles (pairwise different with negatives; small integers, so exact ties, with
// negatives; ties without a negative; all negative), starts up to and past the end, deletions running past the end, zero and
// minus-zero scores.  big_<profile> counts the big lists of a profile with survivors that applied something.
//   usage: greedy_check <checker .so> [trials]
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/poreseq_hip.h"
#include "../../poreseq_amd/csrc/ps_greedy.h"

using ps::Mut;

static unsigned long long rnd_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }
static int below(int n) { return (int)(rnd() % (unsigned long long)n); }
static std::string rseq(int n) { std::string s(n, 'A'); for (char& c : s) c = "ACGT"[below(4)]; return s; }

// One pass of the reference's greedy rule (cpp/MakeMutations.cpp:74-139), restated on the records themselves.  The edits are ranked
// by std::sort, higher score first (the same algorithm on the same comparison results: the reference's order among equal scores),
// and the negative ones, which the ranking puts last, are forgotten.  Then, in rank order: an edit that was set aside goes to
// `aside` with score -1 and the start it has by then; any other edit is spliced into the text and counted with the longer of its
// two sides.  Of the edits ranked behind a spliced one, those with a positive score that come within ten bases of it are set
// aside, untouched; every other one, an earlier set-aside one included, moves by the length change when it starts at or behind the
// end of the replaced bases.
struct Ranked { Mut e; bool aside = false; };

static bool within_spacing(const Mut& done, const Mut& other) {
    const long gap_from = std::max(done.start, other.start);
    const long gap_to = std::min((long)done.start + (long)done.mut.size(), (long)other.start + (long)other.mut.size());
    return gap_from - gap_to < 10;
}

static int plain_pass(std::string& text, const std::vector<Mut>& muts, std::vector<Mut>* aside) {
    std::vector<Mut> order(muts);
    std::sort(order.begin(), order.end(), [](const Mut& x, const Mut& y) { return x.score > y.score; });
    std::vector<Ranked> rank;
    for (const Mut& m : order) if (!(m.score < 0)) { Ranked r; r.e = m; rank.push_back(r); }
    aside->clear();
    int counted = 0;
    for (size_t i = 0; i < rank.size(); i++) {
        if (rank[i].aside) { aside->push_back(rank[i].e); aside->back().score = -1; continue; }
        const Mut done = rank[i].e;
        if ((size_t)done.start < text.size()) text.replace((size_t)done.start, done.orig.size(), done.mut);   // (replace() stops at the end of the text)
        counted += (int)std::max(done.orig.size(), done.mut.size());
        const long behind = (long)done.start + (long)done.orig.size(), grow = (long)done.mut.size() - (long)done.orig.size();
        for (size_t j = i + 1; j < rank.size(); j++) {
            Ranked& r = rank[j];
            if (!r.aside && r.e.score > 0 && within_spacing(done, r.e)) r.aside = true;
            else if (r.e.start >= behind) r.e.start += (int)grow;
        }
    }
    return counted;
}

static bool same_list(const std::vector<Mut>& a, const std::vector<Mut>& b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); k++)
        if (a[k].start != b[k].start || a[k].orig != b[k].orig || a[k].mut != b[k].mut || memcmp(&a[k].score, &b[k].score, sizeof(double))) return false;
    return true;
}

#define SYM(name) decltype(&name) p_##name = (decltype(&name))dlsym(lib, #name); if (!p_##name) { fprintf(stderr, "missing %s\n", #name); return 2; }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: greedy_check <checker .so> [trials]\n"); return 2; }
    void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    SYM(ps_align_create) SYM(ps_align_destroy) SYM(ps_align_sequence_length) SYM(ps_align_get_sequence)
    SYM(ps_muts_create) SYM(ps_muts_destroy) SYM(ps_make_mutations)
    const long trials = argc > 2 ? atol(argv[2]) : 3000;
    static const int sizes[] = {0, 1, 5, 15, 16, 17, 33, 100, 700};
    long bad = 0, deferred = 0, recursed = 0, tied = 0, past_end = 0, big_applied[4] = {0, 0, 0, 0};
    for (long it = 0; it < trials; it++) {
        const int L = 5 + below(396);
        const std::string seq = rseq(L);
        const int profile = (int)(it % 4);
        const bool big = it % 41 == 40;                                    // (41 and 4 share no factor: every profile gets its big lists)
        const int n = big ? 701 + below(2300) : (below(4) == 0 ? below(60) : sizes[below(9)]);
        std::vector<Mut> muts(n);
        for (int k = 0; k < n; k++) {
            Mut& m = muts[k];
            m.start = below(12) == 0 ? L - 2 + below(5) : below(L);      // (up to L + 2: start == len and start > len)
            if (m.start >= L) past_end++;
            m.orig = rseq(below(4));                                       // (only its length counts, cpp/Sequence.h:37-59; may run past the end)
            m.mut = rseq(below(4));
            switch (profile) {
                case 0: m.score = (double)(below(2000001) - 800000) / 1024.0 + 1e-7 * k; break;   // pairwise different (the 1e-7 k term), negatives
                case 1: m.score = (double)(below(9) - 3); break;                                // exact ties, negatives
                case 2: m.score = (double)below(5); break;                                      // ties, no negative
                default: m.score = -(double)(1 + below(4)) * 0.5; break;                        // all negative
            }
            if (profile != 3 && below(50) == 0) m.score = below(2) ? 0.0 : -0.0;
        }
        if (profile == 1 || profile == 2) tied++;
        // the library's loop: passes until at most ten edits are deferred; no events: every re-scored edit gets -1e-6
        std::string got = seq, want = seq;
        int got_nb = 0, want_nb = 0;
        {
            std::vector<Mut> cur = muts, cur_w = muts, later, later_w;
            for (int pass = 0;; pass++) {
                bool changed = false;
                got_nb += ps::greedy_apply(got, cur, &later, false, 0, &changed);
                want_nb += plain_pass(want, cur_w, &later_w);
                if (!same_list(later, later_w) || got != want || got_nb != want_nb) {
                    if (bad++ < 5) printf("trial %ld pass %d (profile %d, %d edits): deferred %zu / %zu, bases %d / %d\n", it, pass, profile, n, later.size(), later_w.size(), got_nb, want_nb);
                    break;
                }
                deferred += (long)later.size();
                if (later.size() <= 10) break;
                recursed++;
                cur = later; cur_w = later_w;
                for (Mut& m : cur) m.score = -1e-6;
                for (Mut& m : cur_w) m.score = -1e-6;
            }
        }
        // the checker library on an AlignData without events
        ps_params par = {4.5, 150, 300, 0};
        const int64_t zero = 0;
        ps_align* h = nullptr;
        if (p_ps_align_create(&h, seq.data(), (int64_t)seq.size(), 0, &zero, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, "", &zero, &par)) { printf("align_create failed\n"); return 2; }
        std::vector<int32_t> start(n + 1);
        std::vector<int64_t> oo(n + 1, 0), mo(n + 1, 0);
        std::vector<double> score(n + 1);
        std::string op, mp;
        for (int k = 0; k < n; k++) {
            start[k] = muts[k].start; score[k] = muts[k].score;
            op += muts[k].orig; mp += muts[k].mut;
            oo[k + 1] = (int64_t)op.size(); mo[k + 1] = (int64_t)mp.size();
        }
        ps_muts* hm = nullptr;
        if (p_ps_muts_create(&hm, n, start.data(), oo.data(), op.c_str(), mo.data(), mp.c_str(), score.data())) { printf("muts_create failed\n"); return 2; }
        int32_t nb = -1;
        if (p_ps_make_mutations(h, hm, &nb)) { printf("make_mutations failed\n"); return 2; }
        std::string out((size_t)p_ps_align_sequence_length(h), '?');
        p_ps_align_get_sequence(h, out.empty() ? nullptr : &out[0], (int64_t)out.size());
        p_ps_muts_destroy(hm);
        p_ps_align_destroy(h);
        if (big && nb > 0) big_applied[profile]++;
        if (nb != got_nb || out != got) { if (bad++ < 5) printf("trial %ld (profile %d, %d edits): checker %d bases, library %d; sequences %s\n", it, profile, n, (int)nb, got_nb, out == got ? "equal" : "differ"); }
    }
    printf("deferred=%ld recursed=%ld tied=%ld past_end=%ld big_distinct_neg=%ld big_ties_neg=%ld big_ties_pos=%ld\n", deferred, recursed, tied, past_end,
           big_applied[0], big_applied[1], big_applied[2]);
    printf("mismatches=%ld\n", bad);
    return bad != 0;
}
