// sw_band_check.cpp — host check of the band mode of the Smith-Waterman fill (poreseq_amd/csrc/ps_sw.hip).  The region of a strip, the
// bound B and the threshold U are the kernels' own: band_win / band_q0 / col_hi, band_bound and band_u of poreseq_amd/csrc/ps_swplan.h.
//
// The fill in band mode computes, for every 512-column strip s, only its rows [512 s + 1 - wb, 512 s + 512 + wb]; every other cell
// counts as 0.  The result is taken only under the certificate the traceback kernel checks: the banded maximum exceeds
// U = 5 max(0, min(n1, n2 - wb - 1), min(n2, n1 - wb - 1)), and every cell the walk reads (the path cell and its left, upper and
// diagonal neighbours, down to the cell where the walk stops) passes Hb >= B, B(i, j) = 5 min(i, j) - 8 max(0, wb + 1 - |i - j|).
// Here a plain full-matrix SW (+5 / -4 / -8, the reference's step order and tie rule) and the banded fill with that certificate run
// on random pairs: whenever the certificate passes, score, start cell and index lists must equal the full SW's; and every cell of the
// banded region with Hb >= B must equal the full value (the bound itself).  Prints the pass rate and "mismatches=N".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../poreseq_amd/csrc/ps_swplan.h"

using namespace ps;

struct Res { int score = 0, bi = 0, bj = 0; std::vector<int> a, b; bool ok = true; };

static int bound(int i, int j, int wb) { return band_bound(i, j, wb); }

static bool in_region(int i, int j, const SwPair& p) {   // 1-based cell (i, j) computed by the band fill: the rows of its strip
    const int s = (j - 1) / SWBS;
    const SwWin w = band_win<true>(p, s);
    return i >= 64 * band_q0<true>(w) + 1 && i <= col_hi<true>(p, w);
}

// wb = 0: the full matrix.  H is (n1 + 1) x (n2 + 1), column-major is not needed: the maximum is searched column by column.
static Res sw(const std::string& s1, const std::string& s2, int wb, std::vector<int32_t>& H) {
    const int n1 = (int)s1.size(), n2 = (int)s2.size(), W = n2 + 1;
    H.assign((size_t)(n1 + 1) * W, 0);
    SwPair p;
    SwPools pools;
    sw_lay_out(p, n1, n2, wb, SW_LISTS, PKK, SWBW, pools);
    auto h = [&](int i, int j) -> int32_t& { return H[(size_t)i * W + j]; };
    for (int i = 1; i <= n1; i++)
        for (int j = 1; j <= n2; j++) {
            if (wb && !in_region(i, j, p)) continue;
            const int d = h(i - 1, j - 1) + (s1[i - 1] == s2[j - 1] ? 5 : -4);
            h(i, j) = std::max(std::max(0, d), std::max(h(i - 1, j) - 8, h(i, j - 1) - 8));
        }
    Res r;
    for (int j = 1; j <= n2; j++)
        for (int i = 1; i <= n1; i++)
            if (h(i, j) > r.score) { r.score = h(i, j); r.bi = i; r.bj = j; }
    if (wb) {
        if (r.score <= band_u(n1, n2, wb)) { r.ok = false; return r; }
    }
    if (r.score <= 0) { r.bi = r.bj = 0; return r; }
    int i = r.bi, j = r.bj;
    while (i > 0 && j > 0) {
        if (wb && !(h(i, j) >= bound(i, j, wb) && h(i, j - 1) >= bound(i, j - 1, wb) && h(i - 1, j) >= bound(i - 1, j, wb) &&
                    h(i - 1, j - 1) >= bound(i - 1, j - 1, wb))) { r.ok = false; return r; }
        if (h(i, j) <= 0) break;
        const int sd = h(i - 1, j - 1) + (s1[i - 1] == s2[j - 1] ? 5 : -4), up = h(i - 1, j) - 8, lf = h(i, j - 1) - 8;
        const int l0 = std::max(lf, 0), m = std::max(l0, up);
        const int step = sd >= m ? 3 : (up > l0 ? 2 : (lf > 0 ? 1 : 0));
        if (step == 3) { r.a.push_back(i); r.b.push_back(j); i--; j--; }
        else if (step == 2) { r.a.push_back(i); r.b.push_back(0); i--; }
        else if (step == 1) { r.a.push_back(0); r.b.push_back(j); j--; }
        else break;
    }
    return r;
}

static std::string rnd(std::mt19937& g, int n) {
    static const char A[] = "ACGT";
    std::string s(n, 'A');
    for (char& c : s) c = A[g() & 3];
    return s;
}

static std::string mutate(std::mt19937& g, const std::string& s, double err) {
    std::uniform_real_distribution<double> u(0, 1);
    std::string o;
    for (char c : s) {
        const double x = u(g);
        if (x < err / 3) continue;                                        // deletion
        if (x < 2 * err / 3) { o.push_back("ACGT"[(g() & 3)]); continue; }   // substitution (possibly silent)
        o.push_back(c);
        if (x < err) o.push_back("ACGT"[g() & 3]);                        // insertion
    }
    return o;
}

int main(int argc, char** argv) {
    const int npairs = argc > 1 ? atoi(argv[1]) : 3000;
    std::mt19937 g(12345);
    std::uniform_real_distribution<double> u(0, 1);
    const int widths[] = {64, 128, 192, 256, 1024};
    long mism = 0, passed = 0, edge = 0, cells_checked = 0;
    std::vector<int32_t> Hf, Hb;
    for (int t = 0; t < npairs; t++) {
        const int wb = widths[t % 5 == 4 && t % 50 == 4 ? 4 : t % 4];
        const bool longp = t % 500 == 7;                                   // a few long pairs (the kernels take up to 13 000)
        const int n = longp ? 3000 + (int)(g() % 3001) : 1 + (int)(g() % (t % 3 ? 1500 : 200));
        const double ident = 0.6 + 0.4 * u(g) * u(g) + (u(g) < 0.5 ? 0.4 * (1 - u(g)) : 0);
        std::string s1 = rnd(g, n), s2 = mutate(g, s1, std::min(1.0, std::max(0.0, 1.0 - ident)));
        const int kind = (int)(g() % 6);
        if (kind == 1) {                                                   // length difference up to 2 wb
            const int d = (int)(g() % (2 * wb + 1));
            if (g() & 1) s1 = rnd(g, d) + s1; else s2 = s2 + rnd(g, d);
        } else if (kind == 2 && n > 40) {                                  // tandem repeat off the diagonal
            const std::string unit = rnd(g, 3 + (int)(g() % 30));
            std::string rep;
            while ((int)rep.size() < 200) rep += unit;
            const int p1 = (int)(g() % s1.size()), p2 = (int)(g() % s2.size());
            s1.insert(p1, rep); s2.insert(p2, rep.substr(0, rep.size() - unit.size() * (g() % 3)));
        } else if (kind == 3 && n > 40) {                                  // interspersed repeat at two offsets
            const std::string rep = rnd(g, 50 + (int)(g() % 400));
            s1.insert((size_t)(g() % s1.size()), rep);
            s2.insert((size_t)(g() % s2.size()), mutate(g, rep, 0.02));
        }
        if (s1.empty() || s2.empty()) continue;
        const Res f = sw(s1, s2, 0, Hf), b = sw(s1, s2, wb, Hb);
        const int n1 = (int)s1.size(), n2 = (int)s2.size(), W = n2 + 1;
        for (int i = 1; i <= n1; i++)                                      // the bound: Hb >= B implies the exact value
            for (int j = 1; j <= n2; j++) {
                const int hb = Hb[(size_t)i * W + j];
                if (hb >= bound(i, j, wb)) {
                    cells_checked++;
                    if (hb != Hf[(size_t)i * W + j]) { if (mism < 10) printf("bound fails: pair %d (%d, %d) wb %d\n", t, i, j, wb); mism++; }
                }
            }
        if (!b.ok) continue;
        passed++;
        if (b.score > 0 && std::abs(b.bi - b.bj) > wb - 64) edge++;
        if (b.score != f.score || b.bi != f.bi || b.bj != f.bj || b.a != f.a || b.b != f.b) {
            if (mism < 10) printf("certified pair differs: pair %d n1 %d n2 %d wb %d score %d / %d\n", t, n1, n2, wb, b.score, f.score);
            mism++;
        }
    }
    printf("pairs=%d certified=%ld (%.1f %%) near_edge=%ld bound_cells=%ld mismatches=%ld\n", npairs, passed, 100.0 * passed / npairs, edge,
           cells_checked, mism);
    return mism ? 1 : 0;
}
