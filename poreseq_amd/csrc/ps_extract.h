// ps_extract.h — the tail of FindMutations for one AlignData on plain host data (cpp/FindMutations.cpp:51-183): likelihood differences
// along the pairwise alignments -> clamped CUSUM -> greedy extraction of candidate edits; and MapAlignments' lookup for one level
// (cpp/EventUtil.cpp:22-51).  No HIP headers
// (tests/native/extract_check.cpp compiles this text with g++ and holds the extraction to a rescan with std::max_element on every
// round, as the reference does); ps_find.cpp feeds it the Smith-Waterman lists and the likelihood vectors that came off the device.
#ifndef PS_EXTRACT_H_
#define PS_EXTRACT_H_

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "ps_greedy.h"   // struct Mut

namespace ps {

constexpr size_t EXTRACT_BLK = 128;   // entries per block maximum

// MapAlignments' lookup for one level (cpp/EventUtil.cpp:22-51): a / b are fillinds' lists of the sequence against a seed, `ra` the
// level's ref_align into the sequence.  -> its ref_align into the seed: b at the first entry of a that is not below ra
// (std::lower_bound), 0 for an empty list or an ra outside [a.front(), a.back()]
inline double map_alignment(const std::vector<int>& a, const std::vector<int>& b, int ra) {
    if (a.empty() || ra < a.front() || ra > a.back()) return 0.0;
    const size_t k = std::lower_bound(a.begin(), a.end(), ra) - a.begin();
    return k < b.size() ? (double)b[k] : 0.0;
}

// cpp/FindMutations.cpp:51-94 for one seed: ia / ib are fillinds' lists of the sequence against the seed (1-based), shifted and
// trimmed in place to valid 0-based indices; base / rl the per-base cumulative likelihoods of the sequence / the seed.  -> the
// clamped CUSUM along the alignment
inline std::vector<double> seed_cusum(std::vector<int>& ia, std::vector<int>& ib, const std::vector<double>& base, const std::vector<double>& rl) {
    for (size_t q = 0; q < ia.size(); q++) { ia[q] -= 2; ib[q] -= 2; }
    while (!ia.empty() && (ia[0] < 0 || ib[0] < 0)) { ia.erase(ia.begin()); ib.erase(ib.begin()); }
    const size_t n = ia.size();
    std::vector<double> x(n), y(n);
    for (size_t q = 0; q < n; q++) {
        x[q] = (size_t)ia[q] < base.size() ? base[ia[q]] : 0.0;
        y[q] = (size_t)ib[q] < rl.size() ? rl[ib[q]] : 0.0;
    }
    for (size_t q = n; q-- > 1;) { x[q] -= x[q - 1]; y[q] -= y[q - 1]; }
    if (n) { x[0] = 0; y[0] = 0; }
    std::vector<double> cs(n);
    double run = 0;
    for (size_t q = 0; q < n; q++) {
        run += y[q] - x[q];
        if (run < 0) run = 0;
        cs[q] = run;
        if (std::fabs(x[q] - y[q]) < 1e-5) cs[q] = 0;
    }
    return cs;
}

// greedy extraction (cpp/FindMutations.cpp:111-183) from the seeds' CUSUM vectors dl (consumed) and their trimmed index lists.  The
// reference rescans every seed's vector for its maximum on each round; here per-seed block maxima (EXTRACT_BLK entries per block)
// are kept current instead — same first-maximum semantics (std::max_element), same output.  Returns 0, or 1 for an alignment index
// outside the sequence.  No seeds: no edits (the reference's loop would index an empty list).
inline int extract_from_cusums(const std::string& bases, const std::vector<std::string>& seeds, const std::vector<std::vector<int>>& ia,
                               const std::vector<std::vector<int>>& ib, std::vector<std::vector<double>>& dl, std::vector<Mut>* out) {
    const size_t L = bases.size();
    const int S = (int)seeds.size();
    if (!S) return 0;
    const size_t BLK = EXTRACT_BLK;
    std::vector<std::vector<double>> bmax(S);
    auto block_refresh = [&](int k, size_t blk) {
        const std::vector<double>& v = dl[k];
        const size_t lo = blk * BLK, hi = std::min(v.size(), lo + BLK);
        double m = v[lo];
        for (size_t q = lo + 1; q < hi; q++) if (v[q] > m) m = v[q];
        bmax[k][blk] = m;
    };
    auto seed_argmax = [&](int k) -> int {   // index of the first maximum of dl[k]
        const std::vector<double>& bm = bmax[k];
        size_t bb = 0;
        for (size_t q = 1; q < bm.size(); q++) if (bm[q] > bm[bb]) bb = q;
        const std::vector<double>& v = dl[k];
        const size_t lo = bb * BLK, hi = std::min(v.size(), lo + BLK);
        size_t at = lo;
        for (size_t q = lo + 1; q < hi; q++) if (v[q] > v[at]) at = q;
        return (int)at;
    };
    std::vector<double> top(S, 0.0);
    std::vector<int> topi(S, 0);
    for (int k = 0; k < S; k++) {
        if (dl[k].empty()) continue;
        bmax[k].resize((dl[k].size() + BLK - 1) / BLK);
        for (size_t blk = 0; blk < bmax[k].size(); blk++) block_refresh(k, blk);
        topi[k] = seed_argmax(k);
        top[k] = dl[k][topi[k]];
    }
    while (out->size() < L / 3) {
        const int w = (int)(std::max_element(top.begin(), top.end()) - top.begin());
        std::vector<double>& v = dl[w];
        if (v.empty()) break;
        const int ind = topi[w];
        if (v[ind] < 0.25) break;
        int i1 = (int)(std::find(v.begin() + ind, v.end(), 0.0) - v.begin());
        int i0 = -1;
        for (int q = ind; q >= 0; q--) if (v[q] == 0) { i0 = q; break; }
        if (i0 < 0) i0 = 0;
        if (i1 < 0) i1 = 0;
        if ((size_t)i0 >= v.size()) i0 = (int)v.size() - 1;
        if ((size_t)i1 >= v.size()) i1 = (int)v.size() - 1;
        const int s1 = ia[w][i0], s2 = ib[w][i0], e1 = ia[w][ind], e2 = ib[w][ind];
        Mut m;
        m.start = s1;
        if ((size_t)s1 > bases.size() || (size_t)s2 > seeds[w].size()) return 1;
        m.orig = bases.substr(s1, (size_t)(e1 - s1));
        m.mut = seeds[w].substr(s2, (size_t)(e2 - s2));
        while (!m.orig.empty() && !m.mut.empty() && m.orig.front() == m.mut.front()) {
            m.orig.erase(m.orig.begin()); m.mut.erase(m.mut.begin()); m.start++;
        }
        while (!m.orig.empty() && !m.mut.empty() && m.orig.back() == m.mut.back()) { m.orig.pop_back(); m.mut.pop_back(); }
        if (!m.orig.empty() || !m.mut.empty()) out->push_back(m);
        std::fill(v.begin() + i0, v.begin() + i1 + 1, 0.0);
        for (size_t blk = (size_t)i0 / BLK; blk <= (size_t)i1 / BLK; blk++) block_refresh(w, blk);
        topi[w] = seed_argmax(w);
        top[w] = v[topi[w]];
    }
    return 0;
}

// the whole tail: bases = the current sequence, seeds[k] with its index lists ia[k] / ib[k] (consumed) and its likelihood vector
// *likes[k]; base = the sequence's own likelihood vector
inline int extract_edits(const std::string& bases, const std::vector<std::string>& seeds, std::vector<std::vector<int>>& ia,
                         std::vector<std::vector<int>>& ib, const std::vector<double>& base, const std::vector<const std::vector<double>*>& likes,
                         std::vector<Mut>* out) {
    const int S = (int)seeds.size();
    std::vector<std::vector<double>> dl(S);
    for (int k = 0; k < S; k++) dl[k] = seed_cusum(ia[k], ib[k], base, *likes[k]);
    return extract_from_cusums(bases, seeds, ia, ib, dl, out);
}

}  // namespace ps
#endif
