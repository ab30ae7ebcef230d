// ps_vitpath.h — the deterministic back-trace of ViterbiMutate (nkeep == 0) over the back-pointer table k_vit_steps leaves behind.
// Pure host code without a dependency: the deterministic tail of viterbi_batch (ps_vit.cpp) and tests/native/vitpath_check.cpp both compile it.
//
// The rule ("Finite outliers"): p[T - 1] = start, p[i - 1] = bp[i][p[i]] for i = T - 1 .. 1.  bp[0][.] is
// never followed, so T = 1 always has a path.  A back-pointer of -1 means that no predecessor of that state scored above -1e300
// (k_vit_steps starts every maximum at -1e300 with back-pointer -1): the state has no path behind it and the walk stops
// there instead of indexing the table with -1.
#pragma once
#include <cstdint>

namespace ps {

// bp_all: rows of `ns` back-pointers, the region's rows at t_off .. t_off + T - 1 (several regions lie concatenated in one table);
// path: T entries.  Returns -1 and the whole path, or the kept position to name in the refusal: from the position i >= 1 where the
// walk met a negative back-pointer, the earliest position j <= i such that every state of rows j .. i - 1 has a negative
// back-pointer too — a dead row kills every later one, so j is the row whose emissions (or running scores) killed the vector.
// path[i .. T - 1] is filled in either case.
inline int64_t vit_follow_bp(const int16_t* bp_all, int64_t t_off, int64_t T, int ns, int start, int* path) {
    int c = start;
    for (int64_t i = T - 1; i >= 0; i--) {
        path[i] = c;
        if (i == 0) break;
        const int q = bp_all[(t_off + i) * ns + c];
        if (q < 0) {
            int64_t j = i;
            for (; j > 0; j--) {
                const int16_t* row = bp_all + (t_off + j - 1) * ns;
                bool dead = true;
                for (int s = 0; s < ns && dead; s++) dead = row[s] < 0;
                if (!dead) break;
            }
            return j;
        }
        c = q;
    }
    return -1;
}

}  // namespace ps
