// ps_greedy.h — one greedy pass of MakeMutations (cpp/MakeMutations.cpp:74-146) on plain host data: the edit record, Sequence(original,
// mut) and the sort / apply / defer / shift loop.  No HIP headers (tests/native/greedy_check.cpp compiles this text with g++ and holds
// it to the checker library, list by list); ps_host.cpp wraps it for an AlignData and re-scores the deferred edits on the device.
#ifndef PS_GREEDY_H_
#define PS_GREEDY_H_

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

namespace ps {

// ---- mutation list (vector<MutInfo>/vector<MutScore>, cpp/AlignUtil.h:69-91) ----------------
struct Mut {
    int start = 0;
    std::string orig, mut;
    double score = -1e-6;
};

// Sequence(original, mut), cpp/Sequence.h:37-59
inline std::string apply_edit(const std::string& b, const Mut& m) {
    if ((size_t)m.start >= b.size()) return b;
    std::string r = b.substr(0, m.start);
    r += m.mut;
    size_t rem = (size_t)m.start + m.orig.size();
    if (rem < b.size()) r += b.substr(rem);
    return r;
}

inline bool by_score_desc(const Mut& x, const Mut& y) { return x.score > y.score; }  // cpp/MakeMutations.cpp:16-17

// MakeMutations, cpp/MakeMutations.cpp:74-146.  std::sort with the same comparator on the same
// libstdc++ gives the reference's (unstable) order for tied scores.
// One greedy pass (host only): sorts, applies the positive edits to `bases`, returns the mutated-base count and the edits that
// were disabled on the way (the reference re-scores and recurses on those when there are more than ten).  *changed: an edit was
// applied (the caller's states are stale); verbose: the AlignData's, for the reference's lines on stderr under `talk`.
inline int greedy_apply(std::string& bases, std::vector<Mut>& muts, std::vector<Mut>* later, bool talk, int verbose, bool* changed) {
    const int spacing = 10;
    int nb = 0;
    later->clear();
    *changed = false;
    {
        // The reference sorts the whole list by descending score and drops the negative tail (cpp/MakeMutations.cpp:80-86).  When
        // the scores that survive (>= 0) are pairwise different — the normal case: a Refine list is 80 000 edits of which a few
        // hundred are positive — their order does not depend on how the rest was permuted, so only they are sorted.  Equal scores
        // among them are ordered by std::sort's own permutation of the WHOLE list, which is then reproduced (index sort: the same
        // comparisons as on the structs, without moving two std::strings per swap).
        std::vector<int> order;
        for (int k = 0; k < (int)muts.size(); k++) if (!(muts[k].score < 0)) order.push_back(k);
        const std::vector<Mut>& mref = muts;
        std::sort(order.begin(), order.end(), [&](int x, int y) { return by_score_desc(mref[x], mref[y]); });
        bool ties = false;
        for (size_t k = 1; k < order.size(); k++) if (muts[order[k - 1]].score == muts[order[k]].score) { ties = true; break; }
        if (ties || order.size() == muts.size()) {
            order.resize(muts.size());
            std::iota(order.begin(), order.end(), 0);
            std::sort(order.begin(), order.end(), [&](int x, int y) { return by_score_desc(mref[x], mref[y]); });
            while (!order.empty() && muts[order.back()].score < 0) order.pop_back();
        }
        std::vector<Mut> kept;
        kept.reserve(order.size());
        for (int k : order) kept.push_back(std::move(muts[k]));
        muts.swap(kept);
    }
    if (muts.empty()) return 0;
    if (talk) { fprintf(stderr, "Testing %zu mutations...\n", muts.size()); fflush(stderr); }   // cpp/MakeMutations.cpp:91-95
    // cpp/MakeMutations.cpp:95-139 with the edits' numbers in flat arrays: the inner loop over all later edits (defer the ones
    // within `spacing` of the applied edit, shift the ones behind it) is then a branch-free integer loop the compiler vectorises —
    // a Mutate list has ~3 000 surviving edits, 4.5 million pair visits per region and call
    const size_t n = muts.size();
    std::vector<int> st(n), ml(n), ol(n), pos(n), dfr(n, 0);
    for (size_t k = 0; k < n; k++) {
        st[k] = muts[k].start; ml[k] = (int)muts[k].mut.size(); ol[k] = (int)muts[k].orig.size();
        pos[k] = muts[k].score > 0 ? 1 : 0;
    }
    for (size_t i = 0; i < n; i++) {
        muts[i].start = st[i];
        if (dfr[i] || muts[i].score < 0) { if (dfr[i]) muts[i].score = -1; later->push_back(muts[i]); continue; }
        bases = apply_edit(bases, muts[i]);
        *changed = true;
        if (talk && verbose > 1) {   // cpp/MakeMutations.cpp:112-118 (operator<< of a double: six significant digits)
            fprintf(stderr, "Kept mutation %zu at %d of %zu to %zu with score %g\n", i, st[i], muts[i].orig.size(), muts[i].mut.size(), muts[i].score);
            fflush(stderr);
        }
        nb += (int)std::max(muts[i].orig.size(), muts[i].mut.size());
        const int si = st[i], ei = si + ml[i], oi = si + ol[i], d = ml[i] - ol[i];
        int* __restrict__ pst = st.data();
        int* __restrict__ ppos = pos.data();
        int* __restrict__ pdf = dfr.data();
        const int* __restrict__ pml = ml.data();
        for (size_t j = i + 1; j < n; j++) {
            const int sj = pst[j];
            const int lo = std::max(si, sj), hi = std::min(ei, sj + pml[j]);
            const int hit = (lo < hi + spacing) & ppos[j];          // overlaps the applied edit (with spacing) and still has a positive score: deferred
            ppos[j] &= ~hit;
            pdf[j] |= hit;
            pst[j] = sj + ((!hit & (sj >= oi)) ? d : 0);            // (a deferred edit keeps its start: the reference `continue`s before the shift)
        }
    }
    return nb;
}

}  // namespace ps
#endif
