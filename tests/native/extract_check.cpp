// Host check of FindMutations' greedy extraction as the library runs it (poreseq_amd/csrc/ps_extract.h: per-seed block maxima of 128
// entries, kept current) against the plain restatement of cpp/FindMutations.cpp:111-183, which rescans every seed's vector with
// std::max_element on every round.  Random CUSUM vectors whose increments are multiples of 0.25, so that equal maxima are common,
// with the situations the block maxima could get wrong planted on purpose and COUNTED (the driving test asserts every count > 0):
//   tie_blocks   the winning seed holds its maximum a second time, in another 128-entry block
//   tie_seeds    another seed's maximum equals the winner's
//   run_span     the run from the previous zero to the maximum crosses a block boundary
//   fill_span    the zero-fill crosses a block boundary
//   no_zero_before / no_zero_after   the maximum has no zero on that side
//   short_vec    the winning vector is shorter than one block
//   empty_vec    a trial with an empty vector among its seeds;  no_seeds: a trial without seeds
// Part 2 runs the whole tail (seed_cusum + extraction) from likelihood vectors and index lists against the same restatement.
// Part 3 holds MapAlignments' lower_bound lookup (map_alignment) to a scan, on named cases and on random lists.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../poreseq_amd/csrc/ps_extract.h"

using ps::Mut;

static unsigned long long rnd_state = 88172645463325252ull;
static unsigned long long rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }
static int below(int n) { return (int)(rnd() % (unsigned long long)n); }
static std::string rseq(int n) { std::string s(n, 'A'); for (char& c : s) c = "ACGT"[below(4)]; return s; }

static long tie_blocks, tie_seeds, run_span, fill_span, no_zero_before, no_zero_after, short_vec, empty_vec, no_seeds;

static int max_index(const std::vector<double>& v) { return (int)(std::max_element(v.begin(), v.end()) - v.begin()); }

// The reference's extraction (cpp/FindMutations.cpp:111-183) restated as a full rescan: every round looks through every seed's whole
// vector for its first maximum (std::max_element; an empty vector stands for 0) and takes the first seed that holds the greatest
// one.  Below 0.25, or when that seed is empty, the list is complete; so it is at a third of the sequence's length.  The edit runs
// from the nearest zero at or before the peak (none: the vector's first entry) to the peak; the vector is cleared from there to
// the nearest zero behind the peak (none: its last entry).  Bases that both sides share are cut off the front, then off the back,
// and what is left empty on both sides is no edit.  `tally` feeds the situation counters.
struct Peak { int seed = -1, at = 0; double value = 0; };

static Peak rescan(const std::vector<std::vector<double>>& cs, bool* shared) {
    Peak best;
    *shared = false;
    for (size_t k = 0; k < cs.size(); k++) {
        const int at = cs[k].empty() ? 0 : max_index(cs[k]);
        const double value = cs[k].empty() ? 0.0 : cs[k][at];
        if (best.seed < 0 || value > best.value) { best.seed = (int)k; best.at = at; best.value = value; *shared = false; }
        else if (value == best.value) *shared = true;
    }
    return best;
}

static void naive_extract(const std::string& bases, const std::vector<std::string>& seeds, const std::vector<std::vector<int>>& ia,
                          const std::vector<std::vector<int>>& ib, std::vector<std::vector<double>> cs, std::vector<Mut>* out, bool tally) {
    const size_t cap = bases.size() / 3;
    while (!cs.empty() && out->size() < cap) {
        bool shared = false;
        const Peak pk = rescan(cs, &shared);
        std::vector<double>& v = cs[pk.seed];
        if (v.empty() || pk.value < 0.25) return;
        const int last = (int)v.size() - 1;
        int left = pk.at, right = pk.at;
        while (left >= 0 && v[left] != 0) left--;
        while (right <= last && v[right] != 0) right++;
        if (tally) {
            for (int q = 0; q <= last; q++) if (v[q] == pk.value && q / 128 != pk.at / 128) { tie_blocks++; break; }
            tie_seeds += shared;
            no_zero_before += left < 0;
            no_zero_after += right > last;
            short_vec += last + 1 < 128;
        }
        left = std::max(left, 0);
        right = std::min(right, last);
        if (tally) { run_span += left / 128 != pk.at / 128; fill_span += left / 128 != right / 128; }
        const std::vector<int>& pa = ia[pk.seed];
        const std::vector<int>& pb = ib[pk.seed];
        const std::string from = bases.substr(pa[left], pa[pk.at] - pa[left]);
        const std::string to = seeds[pk.seed].substr(pb[left], pb[pk.at] - pb[left]);
        size_t head = 0, tail = 0;
        while (head < from.size() && head < to.size() && from[head] == to[head]) head++;
        while (head + tail < from.size() && head + tail < to.size() && from[from.size() - 1 - tail] == to[to.size() - 1 - tail]) tail++;
        Mut e;
        e.start = pa[left] + (int)head;
        e.orig = from.substr(head, from.size() - head - tail);
        e.mut = to.substr(head, to.size() - head - tail);
        if (!e.orig.empty() || !e.mut.empty()) out->push_back(e);
        for (int q = left; q <= right; q++) v[q] = 0;
    }
}

// The reference's CUSUM of one seed (cpp/FindMutations.cpp:51-94) restated: the 1-based pairs become 0-based indices of the bases
// two further back, and the leading pairs that then point before either sequence are dropped (-> ka / kb).  Along the rest, the
// seed's likelihood increment minus the sequence's is summed and clamped at zero; the first entry has no increment, and an entry
// whose two increments differ by less than 1e-5 is zero whatever the sum says.
static std::vector<double> naive_cusum(const std::vector<int>& a, const std::vector<int>& b, const std::vector<double>& base,
                                       const std::vector<double>& seedlk, std::vector<int>* ka, std::vector<int>* kb) {
    size_t first = 0;
    while (first < a.size() && (a[first] < 2 || b[first] < 2)) first++;
    ka->clear(); kb->clear();
    for (size_t q = first; q < a.size(); q++) { ka->push_back(a[q] - 2); kb->push_back(b[q] - 2); }
    std::vector<double> cs(ka->size(), 0.0);
    double sum = 0;
    for (size_t q = 1; q < cs.size(); q++) {
        const double own = base[(*ka)[q]] - base[(*ka)[q - 1]];
        const double theirs = seedlk[(*kb)[q]] - seedlk[(*kb)[q - 1]];
        sum = std::max(sum + (theirs - own), 0.0);
        cs[q] = std::fabs(own - theirs) < 1e-5 ? 0.0 : sum;
    }
    return cs;
}

// MapAlignments' rule for one level (cpp/EventUtil.cpp:22-51) restated as a scan: a level whose ref_align lies within the range of the
// sequence's list goes to the seed's index at the first pair whose sequence index has reached it; any other level is not aligned (0)
static double naive_map(const std::vector<int>& a, const std::vector<int>& b, int ra) {
    if (a.empty() || ra < a[0] || ra > a[a.size() - 1]) return 0.0;
    for (size_t k = 0; k < a.size(); k++) if (a[k] >= ra) return (double)b[k];
    return 0.0;
}

static bool same(const std::vector<Mut>& a, const std::vector<Mut>& b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); k++) if (a[k].start != b[k].start || a[k].orig != b[k].orig || a[k].mut != b[k].mut) return false;
    return true;
}

// monotone index lists of length n into sequences of L1 / L2 bases (base0 = 0: 0-based; > 0: as before the shift by 2), steps of 0 (a gap, as fillinds leaves it), 1 or rarely 2
static void lists(int n, int L1, int L2, int base0, std::vector<int>* a, std::vector<int>* b) {
    a->resize(n); b->resize(n);
    int x = base0, y = base0;
    for (int q = 0; q < n; q++) {
        (*a)[q] = std::min(x, L1 - 1 + (base0 ? 2 : 0)); (*b)[q] = std::min(y, L2 - 1 + (base0 ? 2 : 0));
        const int r = below(20);
        if (r == 0) x++; else if (r == 1) y++; else if (r == 2) { x += 2; y++; } else { x++; y++; }
    }
}

int main(int argc, char** argv) {
    const long trials = argc > 1 ? atol(argv[1]) : 4000;
    long bad = 0;
    for (long it = 0; it < trials; it++) {
        const int S = it % 37 == 0 ? 0 : 1 + below(4);
        if (!S) no_seeds++;
        const int nmax = it % 3 == 0 ? 100 : (it % 3 == 1 ? 300 : 700);
        const int L = 5 + below(nmax + 200);
        const std::string bases = rseq(L);
        std::vector<std::string> seeds(S);
        std::vector<std::vector<int>> ia(S), ib(S);
        std::vector<std::vector<double>> dl(S);
        bool any_empty = false;
        for (int k = 0; k < S; k++) {
            const int n = below(11) == 0 ? 0 : 1 + below(nmax);
            const int L2 = 5 + below(nmax + 200);
            seeds[k] = rseq(L2);
            lists(n, L, L2, 0, &ia[k], &ib[k]);
            any_empty |= n == 0;
            // clamped walk in steps of 0.25: `calm` walks reset to zero often, the others run for hundreds of entries
            const bool calm = below(3) == 0;
            double run = below(4) == 0 ? 0.25 * (1 + below(6)) : 0.0;      // (a first entry > 0: no zero before the maximum)
            std::vector<double>& v = dl[k];
            v.resize(n);
            for (int q = 0; q < n; q++) {
                if (q) {
                    const int r = below(calm ? 8 : 64);
                    if (r == 0) run = 0;
                    else run += 0.25 * (below(7) - 3);
                    if (run < 0) run = 0;
                    if (run > 3.0) run = 3.0 - 0.25 * below(3);             // a low ceiling: the maximum is reached many times
                }
                v[q] = run;
            }
        }
        if (S > 1 && below(3) == 0) {   // the same maximum in two seeds
            const int a = below(S), b = (a + 1 + below(S - 1)) % S;
            if (!dl[a].empty() && !dl[b].empty()) dl[b][below((int)dl[b].size())] = dl[a][max_index(dl[a])];
        }
        if (S && any_empty) empty_vec++;
        std::vector<Mut> got, want;
        std::vector<std::vector<double>> work(dl);
        const int rc = ps::extract_from_cusums(bases, seeds, ia, ib, work, &got);
        naive_extract(bases, seeds, ia, ib, dl, &want, true);
        if (rc != 0 || !same(got, want)) { if (bad++ < 5) printf("trial %ld: rc %d, %zu edits, want %zu\n", it, rc, got.size(), want.size()); }
    }
    // 2. the whole tail from likelihood vectors: cumulative sums in steps of 0.25 (exact), lists 1-based with the leading entries
    //    that the shift by 2 makes invalid
    for (long it = 0; it < trials / 4 + 20; it++) {
        const int S = 1 + below(4), L = 6 + below(500);
        const std::string bases = rseq(L);
        std::vector<double> base(L, 0.0);
        for (int q = 1; q < L; q++) base[q] = base[q - 1] + 0.25 * (below(9) - 2);
        std::vector<std::string> seeds(S);
        std::vector<std::vector<double>> lk(S);
        std::vector<const std::vector<double>*> lkp(S);
        std::vector<std::vector<int>> ia(S), ib(S);
        for (int k = 0; k < S; k++) {
            const int L2 = 6 + below(500), n = below(9) == 0 ? below(3) : 1 + below(std::min(L, L2) + 20);
            seeds[k] = rseq(L2);
            lk[k].assign(L2, 0.0);
            for (int q = 1; q < L2; q++) lk[k][q] = lk[k][q - 1] + 0.25 * (below(9) - 2) + (below(40) == 0 ? 1e-6 : 0.0);
            lkp[k] = &lk[k];
            lists(n, L, L2, 1 + below(3), &ia[k], &ib[k]);
        }
        std::vector<std::vector<int>> na(S), nb(S);
        std::vector<std::vector<double>> dl(S);
        for (int k = 0; k < S; k++) dl[k] = naive_cusum(ia[k], ib[k], base, lk[k], &na[k], &nb[k]);
        std::vector<Mut> got, want;
        const int rc = ps::extract_edits(bases, seeds, ia, ib, base, lkp, &got);
        naive_extract(bases, seeds, na, nb, dl, &want, false);
        if (rc != 0 || !same(got, want) || ia != na || ib != nb) { if (bad++ < 5) printf("whole tail, trial %ld: rc %d, %zu edits, want %zu\n", it, rc, got.size(), want.size()); }
    }
    // 3. MapAlignments' lookup (cpp/EventUtil.cpp:22-51) against its restatement, on the cases named there and on random lists
    {
        const std::vector<int> none, a = {3, 4, 4, 4, 7, 9, 9, 12}, b = {10, 11, 12, 13, 14, 15, 16, 17};
        struct { const std::vector<int>* a; const std::vector<int>* b; int ra; double want; } cases[] = {
            {&none, &none, 5, 0.0},    // an empty list
            {&a, &b, 2, 0.0},          // below the first entry
            {&a, &b, 13, 0.0},         // above the last
            {&a, &b, 3, 10.0},         // the first entry itself
            {&a, &b, 4, 11.0},         // a repeated index: the first of its entries
            {&a, &b, 5, 14.0},         // between two entries: the next one up (7) ...
            {&a, &b, 8, 15.0},         // ... and of a repeated one (9) the first
            {&a, &b, 12, 17.0},        // a hit on the last entry
            {&a, &b, 0, 0.0},          // ref_align of a level that is not aligned
        };
        for (const auto& c : cases) {
            const double got = ps::map_alignment(*c.a, *c.b, c.ra);
            if (got != c.want || got != naive_map(*c.a, *c.b, c.ra)) { if (bad++ < 5) printf("map_alignment(%d): %g, want %g\n", c.ra, got, c.want); }
        }
    }
    for (long it = 0; it < trials; it++) {
        std::vector<int> a, b;
        lists(below(40), 30, 30, 1 + below(3), &a, &b);
        for (int ra = -1; ra < 36; ra++)
            if (ps::map_alignment(a, b, ra) != naive_map(a, b, ra)) { if (bad++ < 5) printf("map_alignment, trial %ld: ra %d\n", it, ra); }
    }
    printf("tie_blocks=%ld tie_seeds=%ld run_span=%ld fill_span=%ld no_zero_before=%ld no_zero_after=%ld short_vec=%ld empty_vec=%ld no_seeds=%ld\n",
           tie_blocks, tie_seeds, run_span, fill_span, no_zero_before, no_zero_after, short_vec, empty_vec, no_seeds);
    printf("mismatches=%ld\n", bad);
    return bad != 0;
}
