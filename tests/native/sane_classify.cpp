// sane_classify.cpp — test program (tests/edge_cases.py, host_verdict): what ps_align_create decides about the tables of one
// AlignData, by the header the library decides with (poreseq_amd/csrc/ps_sane.h).  Standard input: one record per line in
// hexadecimal floats — "L mean stdv" for an event level, "M level_mean level_stdv sd_mean sd_stdv" for a model row,
// "P lik_offset".  Answer: "refused" (a +infinity emission: ps_align_create fails), else "marked" (emissions of -infinity or NaN:
// ViterbiMutate refuses the AlignData) or "unmarked", then "ieee" (some value outside the tabulated range) or "fast".
#include <cstdio>
#include <cstdlib>

#include "../../poreseq_amd/csrc/ps_sane.h"

int main() {
    char kind[8], a[64], b[64], c[64], d[64];
    bool fast = true, refused = false, marked = false;
    long n = 0;
    while (std::scanf("%7s %63s", kind, a) == 2) {
        n++;
        const double va = std::strtod(a, nullptr);
        if (kind[0] == 'P') { refused |= ps::offset_refused(va); continue; }
        if (std::scanf("%63s", b) != 1) return 2;
        const double vb = std::strtod(b, nullptr);
        if (kind[0] == 'L') {
            refused |= ps::level_plus_inf(vb);
            marked |= ps::level_nonfinite(va, vb);
            fast &= ps::sane_level(va, vb);
        } else {
            if (std::scanf("%63s %63s", c, d) != 2) return 2;
            const double sm = std::strtod(c, nullptr), lam = ps::model_lambda(sm, std::strtod(d, nullptr));
            refused |= ps::model_row_plus_inf(vb, lam);
            marked |= ps::model_row_nonfinite(va, vb, sm, lam);
            fast &= ps::sane_model_row(va, vb, sm, lam);
        }
    }
    std::printf("%s %s records=%ld\n", refused ? "refused" : marked ? "marked" : "unmarked", fast ? "fast" : "ieee", n);
    return 0;
}
