// remap_check.cpp — host check of poreseq_amd/csrc/ps_remap.h (the text k_remap compiles) against PSEvent.mapaligns.
//
//   remap_check FILE        FILE: per case   n m / inds1[n] / inds2[n] / x[m] (hex floats) / expected[m] (hex floats)
//
// For every case the partner table and its record are built from the index lists the way the SW_MAP traceback does — in WALK order,
// i.e. from the lists' last entry to their first: a non-zero seq1 index writes its table entry and moves lo (the first one met is
// hi), an entry with inds1 == 0 sets has0 and overwrites y0 — and remap_level is compared, bit for bit, with what the Python rule
// gave for each x.  Prints  cases=.. levels=.. interpolated=.. mismatches=..
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../poreseq_amd/csrc/ps_remap.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    long cases = 0, levels = 0, interp = 0, bad = 0;
    int n, m;
    while (fscanf(f, "%d %d", &n, &m) == 2) {
        std::vector<int> a(n), b(n);
        std::vector<double> x(m), want(m);
        for (int k = 0; k < n; k++) if (fscanf(f, "%d", &a[k]) != 1) return 3;
        for (int k = 0; k < n; k++) if (fscanf(f, "%d", &b[k]) != 1) return 3;
        char tok[64];
        for (int k = 0; k < m; k++) { if (fscanf(f, "%63s", tok) != 1) return 3; x[k] = strtod(tok, nullptr); }
        for (int k = 0; k < m; k++) { if (fscanf(f, "%63s", tok) != 1) return 3; want[k] = strtod(tok, nullptr); }
        int top = 0;
        for (int k = 0; k < n; k++) top = a[k] > top ? a[k] : top;
        std::vector<int> part(top + 2, -12345);   // (entries the walk does not write must never be read)
        ps::RemapRec r = {0, 0, 0, 0};
        for (int k = n - 1; k >= 0; k--) {
            if (a[k] > 0) { part[a[k]] = b[k]; if (!r.hi) r.hi = a[k]; r.lo = a[k]; }
            else { r.has0 = 1; r.y0 = b[k]; }
        }
        for (int k = 0; k < m; k++) {
            const double got = ps::remap_level(x[k], part.data(), r);
            if (x[k] > 0 && x[k] < r.lo && r.has0) interp++;
            if (memcmp(&got, &want[k], sizeof(double)) != 0 && !(got == 0.0 && want[k] == 0.0)) {
                if (bad < 10) fprintf(stderr, "case %ld: x = %a: got %a, want %a (lo %d hi %d has0 %d y0 %d)\n", cases, x[k], got, want[k], r.lo, r.hi, r.has0, r.y0);
                bad++;
            }
        }
        cases++; levels += m;
    }
    fclose(f);
    printf("cases=%ld levels=%ld interpolated=%ld mismatches=%ld\n", cases, levels, interp, bad);
    return bad ? 1 : 0;
}
