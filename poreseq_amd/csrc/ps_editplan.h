// ps_editplan.h — the host arithmetic of an edit-scoring call on plain data: the 5-mer states of a sequence, FindPointMutations' list
// and its per-position layout, and the plan of an edit list (sizes, new columns and their states, kept matrix columns, distinct old-score
// columns, size classes) that k_old / k_score read.  No HIP headers (tests/native/editplan_check.cpp compiles this text with g++ and
// holds every table to a naive restatement on whole edited sequences); ps_score.cpp stages the tables for the device.
#ifndef PS_EDITPLAN_H_
#define PS_EDITPLAN_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "../../include/poreseq_hip.h"
#include "ps_greedy.h"   // struct Mut

namespace ps {

constexpr int NS = PS_N_STATES;
constexpr int PT_SLOTS = 9;    // deletion, substitution by A / C / G / T, insertion of A / C / G / T
// k_score is built for five group sizes; an edit goes to the smallest that holds its new columns.  Class k < 4 fits 8 << k lanes
// (k = 3: chunked, any size), class 4 fits 7 (point edits, len(mut) <= 1: 6 or 7 new columns — nine edits to a wave instead of eight)
constexpr int SCORE_CLASSES = 5;
constexpr int score_class(int ncol) { return ncol <= 7 ? 4 : ncol <= 8 ? 0 : ncol <= 16 ? 1 : ncol <= 32 ? 2 : 3; }
constexpr int score_class_lanes(int k) { return k == 4 ? 7 : 8 << k; }

// Sequence::populateStates, cpp/Sequence.h:64-100
inline std::vector<int> states_of(const std::string& bases) {
    std::vector<int> st;
    if (bases.size() < 5) return st;
    auto code = [](char c) -> int { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : (int)(signed char)c; };
    // (shifted as unsigned: a byte >= 0x80 has a negative code, and what it leaves in `cur` is shifted on — the same bits, defined)
    auto shift_in = [](int cur, int c) -> int { return (int)(((unsigned)cur << 2) + (unsigned)c); };
    int cur = 0;
    for (int i = 0; i < 4; i++) cur = shift_in(cur, code(bases[i]));
    st.resize(bases.size() - 4);
    for (size_t i = 4; i < bases.size(); i++) {
        if (code(bases[i - 4]) < 4) { cur = (NS - 1) & shift_in(cur, code(bases[i])); st[i - 4] = cur; }
        else { cur = 0; st[i - 4] = -1; }
    }
    return st;
}

// states of the edited sequence at columns sidx+1 .. sidx+ncol, without building the whole sequence;
// equals Sequence(original, mut).states there (cpp/Sequence.h:37-100).  A 12-base look-back flushes
// every effect of earlier non-ACGT characters (they reach at most 8 states ahead).
inline void edited_window(const std::string& b, const Mut& m, int sidx, int ncol, int* out) {
    const bool copy = (size_t)m.start >= b.size();
    const int64_t L = (int64_t)b.size();
    const int64_t cut = copy ? L : std::min<int64_t>(L, (int64_t)m.start + (int64_t)m.orig.size());
    const int64_t mlen = copy ? 0 : (int64_t)m.mut.size();
    const int64_t Lm = copy ? L : (int64_t)m.start + mlen + (L - cut);
    auto at = [&](int64_t p) -> char {
        if (copy || p < m.start) return b[p];
        if (p < m.start + mlen) return m.mut[p - m.start];
        return b[cut + (p - m.start - mlen)];
    };
    const int64_t lo = std::max<int64_t>(0, (int64_t)sidx - 12);
    const int64_t hi = std::min<int64_t>(Lm, (int64_t)sidx + ncol + 4);
    std::string w;
    w.reserve(hi - lo);
    for (int64_t p = lo; p < hi; p++) w.push_back(at(p));
    std::vector<int> st = states_of(w);
    for (int c = 0; c < ncol; c++) {
        const int64_t k = (int64_t)sidx + c - lo;
        out[c] = (k >= 0 && k < (int64_t)st.size()) ? st[k] : -1;
    }
}

// FindPointMutations' list, cpp/FindMutations.cpp:200-228, for the first npos positions of `bases`
inline void point_edits(const std::string& bases, size_t npos, std::vector<Mut>* out) {
    static const char B4[] = "ACGT";
    out->clear();
    out->reserve(npos * 8);
    for (size_t i = 0; i < npos; i++) {
        Mut m;
        m.start = (int)i;
        m.orig.assign(1, bases[i]);
        out->push_back(m);
        for (int k = 0; k < 4; k++) {
            if (bases[i] == B4[k]) continue;
            m.mut.assign(1, B4[k]);
            out->push_back(m);
        }
        m.orig.clear();
        for (int k = 0; k < 4; k++) { m.mut.assign(1, B4[k]); out->push_back(m); }
    }
}

// Where that list keeps each position's edits: first[p] is the index of position p's deletion, followed by its substitutions in
// ACGT order without the one by the base itself, then the four insertions — 8 edits for an A / C / G / T base, 9 for any other
// character; first[n] = the length of the list.  triv[p]: table slot 1 .. 4 of the substitution that is not in the list, 0 when
// all four are.
inline void point_layout(const std::string& bases, size_t npos, std::vector<int>* first, std::vector<int>* triv) {
    first->resize(npos + 1); triv->resize(npos);
    int m = 0;
    for (size_t i = 0; i < npos; i++) {
        const char c = bases[i];
        const int t = c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 3 : c == 'T' ? 4 : 0;
        (*first)[i] = m; (*triv)[i] = t;
        m += t ? 8 : 9;
    }
    (*first)[npos] = m;
}

// the rows of an AlignData without events: every edit keeps the seed of its sum, -1e-6 (cpp/AlignUtil.h:86)
inline void point_rows_seed(const std::vector<int>& triv, double* table, ps_point_best* best) {
    for (size_t p = 0; p < triv.size(); p++) {
        if (table)
            for (int q = 0; q < PT_SLOTS; q++) table[p * PT_SLOTS + q] = (triv[p] && q == triv[p]) ? std::nan("") : -1e-6;
        if (best) { best[p].margin = -1e-6; best[p].slot = 0; best[p].n_positive = 0; }
    }
}

// host-side description of one AlignData's edit list for k_old / k_score; `bases` is its sequence, C its states, WS its scoring_width
struct EditPlan {
    int M = 0, ncolmax = 1, extra = 0, nr0 = 0;
    std::vector<int> start, mlen, cm, ncol, skip, oldidx, states, r0s, cls[SCORE_CLASSES];
    std::vector<int> keep[2];   // per direction: kept-column index of column 0 .. C + 1, or -1 (plan_keep)
    int nkeep[2] = {0, 0};
    bool bad_start = false;     // an edit starts below 0: nothing else was planned
};

inline void plan_edits(const std::string& bases, int C, int WS, const std::vector<Mut>& muts, EditPlan* p) {
    const int M = (int)muts.size();
    p->M = M;
    for (const Mut& m : muts) if (m.start < 0) { p->bad_start = true; return; }
    const int64_t L = (int64_t)bases.size();
    p->start.resize(M); p->mlen.resize(M); p->cm.resize(M); p->ncol.resize(M); p->skip.resize(M); p->oldidx.resize(M);
    int ncolmax = 1, extra = 0;
    for (int i = 0; i < M; i++) {
        const Mut& m = muts[i];
        p->start[i] = m.start; p->mlen[i] = (int)m.mut.size();
        p->skip[i] = (int64_t)m.start > L ? 1 : 0;  // "sanity check", cpp/MakeMutations.cpp:46-47
        const bool copy = (int64_t)m.start >= L;
        const int64_t cut = std::min<int64_t>(L, (int64_t)m.start + (int64_t)m.orig.size());
        const int64_t Lm = copy ? L : (int64_t)m.start + (int64_t)m.mut.size() + (L - cut);
        const int Cm = Lm >= 5 ? (int)(Lm - 4) : 0;
        p->cm[i] = Cm;
        const int sidx = std::max(m.start - 4, 0);
        int ncol = std::min<int64_t>((int64_t)m.mut.size() + 6, std::max<int64_t>(0, (int64_t)Cm - sidx));
        if (WS == 0 || p->skip[i]) ncol = 0;  // stripe_width 0 makes fillColumn a no-op, cpp/Alignment.cpp:118-119
        p->ncol[i] = ncol;
        ncolmax = std::max(ncolmax, ncol);
        if (!p->skip[i]) extra = std::max(extra, sidx + ncol + 1 - (C + 1));
    }
    p->ncolmax = ncolmax;
    p->extra = std::max(extra, 0) + 2;
}

// The matrix columns the scoring of this list will read (k_old / k_score, cpp/Alignment.cpp:447-512, cpp/Alignment.h:181-214):
// per edit the forward column it is spliced behind, max(start - 4, 0), the column pair of its old score, max(start - 3, 1) forward
// and C - that + 1 backward, and the backward column its target is combined with — with the kernels' own clamping.  Column 0 (the
// blank column) is never read from the records.
inline void plan_keep(int C, EditPlan* p) {
    for (int d = 0; d < 2; d++) { p->keep[d].assign((size_t)C + 2, -1); p->nkeep[d] = 0; }
    auto clampc = [&](int c) { return (unsigned)c >= (unsigned)(C + 1) ? C : c; };
    for (int i = 0; i < p->M; i++) {
        if (p->skip[i]) continue;
        const int start = p->start[i];
        const int sidx = std::max(start - 4, 0);
        const int tcol = std::min(start + p->mlen[i] + 1, sidx + p->ncol[i]);
        const int backind = clampc(p->cm[i] - tcol + 1);
        const int r0 = std::max(start - 3, 1);
        const int raf = clampc(r0), rab = clampc(C - r0 + 1);
        const int sf = clampc(sidx);
        if (sf > 0) p->keep[0][sf] = 0;
        if (raf > 0) p->keep[0][raf] = 0;
        if (backind > 0) p->keep[1][backind] = 0;
        if (rab > 0) p->keep[1][rab] = 0;
    }
    for (int d = 0; d < 2; d++)
        for (int c = 0; c <= C + 1; c++) if (p->keep[d][c] == 0) p->keep[d][c] = p->nkeep[d]++;
}

// second half of the plan (runs on host threads while the GPU realigns): edited states, distinct r0, size classes
inline void plan_tables(const std::string& bases, const std::vector<Mut>& muts, EditPlan* p, int nth) {
    const int M = p->M, ncolmax = p->ncolmax;
    const int64_t L = (int64_t)bases.size();
    p->states.assign((size_t)M * ncolmax, -1);
    {
        auto work = [&](int lo, int hi) {
            for (int i = lo; i < hi; i++)
                if (p->ncol[i] > 0) edited_window(bases, muts[i], std::max(muts[i].start - 4, 0), p->ncol[i], p->states.data() + (size_t)i * ncolmax);
        };
        if (M < 4096) nth = 1;   // Refine-sized lists: split over a few host threads (disjoint outputs)
        std::vector<std::thread> th;
        for (int t = 1; t < nth; t++) th.emplace_back(work, (int)((int64_t)M * t / nth), (int)((int64_t)M * (t + 1) / nth));
        work(0, (int)((int64_t)M / nth));
        for (std::thread& x : th) x.join();
    }
    std::vector<int> idx((size_t)std::max<int64_t>(L, 4) + 2, -1);   // r0 <= L - 3 for every edit that is not skipped
    for (int i = 0; i < M; i++) {
        if (p->skip[i]) { p->oldidx[i] = 0; continue; }
        const int r0 = std::max(muts[i].start - 3, 1);
        int& at = idx[r0];
        if (at < 0) { at = (int)p->r0s.size(); p->r0s.push_back(r0); }
        p->oldidx[i] = at;
    }
    p->nr0 = (int)p->r0s.size();
    for (int i = 0; i < M; i++) p->cls[score_class(p->ncol[i])].push_back(i);
}

}  // namespace ps
#endif
